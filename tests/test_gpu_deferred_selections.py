"""GPU: the deferred selections of a forward (forward.hip, side_queries: fp1's 3-NN, the regressors' samplings and both hands' ball
queries wait on the side stream for enc.sa3 and run beside the dense layers of fp3 and fp2) against the single-stream forward
(ev2h_set_side_stream(0): everything in program order on one stream), bit for bit, and against stale reads.  A consumer that misses
the EV_ENC_SA3 / EV_FP1_NN / EV_HAND_QUERIES edges reads what the LAST forward left in the workspace, which is invisible while every
forward sees the same input: so the inputs alternate and the whole workspace is overwritten with 0xFF bytes between two forwards --
eagerly, as a hipGraph replay (one more cross-stream edge in the capture), and with two forwards in flight.

Shapes: 64 windows, the edge of the gate, of 1024 and 2048 points, f16x2 and bf16; the same windows at the head of a 96-window batch;
and 8 and 32 windows, which keep the earlier order.  Everything is computed once (module fixture); the tests compare what it saved."""
import pytest
import torch

from ev2hands_amd import _lib, synth
from ev2hands_amd.inflight import InflightForward

pytestmark = pytest.mark.gpu

CASES = [("f16x2", 64, 1024), ("f16x2", 64, 2048), ("bf16", 64, 1024), ("bf16", 64, 2048)]
UNGATED = [("f16x2", 8, 2048), ("f16x2", 32, 2048)]
BIG = 96
ROUNDS = 3
SELECTIONS = ("nn1_idx", "fpsmL", "fpsmR", "gidxm0L", "gidxm1L", "gidxm0R", "gidxm1R", "cntmL", "cntmR")


def flat(o):
    return {"class_logits": o["class_logits"].clone(),
            **{f"{s}.{k}": o[s][k].clone() for s in ("left", "right") for k in ("vertices", "j3d", "global_orient", "hand_pose", "betas", "transl")}}


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in b)


def forward(net, xyz, inits):
    net.net.fps_init = inits
    with torch.no_grad():
        o = flat(net(xyz))
    torch.cuda.synchronize()
    return o


def single_stream(net, xyz, inits):
    prev = _lib.lib().ev2h_set_side_stream(0)
    try:
        return forward(net, xyz, inits)
    finally:
        _lib.lib().ev2h_set_side_stream(prev)


@pytest.fixture(scope="module")
def runs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import os
    from ev2hands_amd.model import TEHNetWrapper
    os.environ["ERPC"] = "0"
    assets = {s: synth.synth_mano_assets(s, 4) for s in ("left", "right")}
    sd = synth.synth_state_dict(4, 4)

    def make(prec):
        net = TEHNetWrapper("cuda:0", mano_assets=assets, precision=prec)
        net.load_state_dict(sd, strict=True)
        net.eval()
        return net

    res = {}
    clouds = {}
    for prec, B, N in CASES + UNGATED:
        if N not in clouds:          # BIG windows of two inputs X, Y; a batch of B is their first B windows, with the same start indices
            clouds[N] = [(synth.synth_cloud("E", BIG, 4, N, 21 + i).cuda(), synth.fps_inits(BIG, N, 21 + i)) for i in range(2)]
        inp = [(x[:B].contiguous(), [v[:B].contiguous() for v in ini]) for x, ini in clouds[N]]
        r = res[(prec, B, N)] = {}
        # the single-stream forward of a fresh model (its own workspace) per input: what everything else must equal
        want = [single_stream(make(prec), *inp[i]) for i in range(2)]
        fresh = make(prec)
        r["two_streams"] = [same(forward(fresh, *inp[i]), want[i]) for i in range(2)]
        # the deferred selections are real ones, not two equal poisoned buffers: indices of points of the window
        r["selections"] = {n: (int(v.min()), int(v.max())) for n in SELECTIONS for v in [fresh.net.debug_buffer(n, torch.int32)]}
        if (prec, B, N) in UNGATED:
            continue
        net = make(prec)
        big = forward(net, *clouds[N][0])
        r["in_batch"] = all(torch.equal(big[k][:B], want[0][k]) for k in want[0])
        # eager: forward, poison the whole workspace, forward on the other input
        forward(net, *inp[0])
        ok = []
        for k in range(ROUNDS):
            net.net._ws.fill_(0xFF)
            ok.append(same(forward(net, *inp[(k + 1) & 1]), want[(k + 1) & 1]))
        r["eager"] = ok
        net.net._ws.fill_(0xFF)
        r["single_stream"] = [same(single_stream(net, *inp[i]), want[i]) for i in range(2)]
        # hipGraph: captured once, replayed on refreshed static inputs
        g = net.net.capture(inp[0][0], net.hands, inp[0][1])
        ok = []
        for k in range(ROUNDS):
            torch.cuda.synchronize()
            g._ws.fill_(0xFF)
            o = g.replay(*inp[(k + 1) & 1])
            torch.cuda.synchronize()
            ok.append(same(flat(o), want[(k + 1) & 1]))
        r["graph"] = ok
        del g
        # two forwards in flight, each slot with its own workspace and side stream
        pipe = InflightForward(net, 2)
        ok = []
        for k in range(ROUNDS + 1):
            order = [(k + j) & 1 for j in range(2)]
            tickets = []
            for i in order:
                net.net.fps_init = inp[i][1]
                tickets.append(pipe.submit(inp[i][0]))
            outs = [flat(t.result()) for t in tickets]
            pipe.drain()
            torch.cuda.synchronize()
            if k:                                                   # (round 0 fills the slots' workspaces with real values to go stale)
                ok.append(all(same(o, want[i]) for o, i in zip(outs, order)))
            for w in pipe.ws:
                w.fill_(0xFF)
        r["inflight"] = ok
        del pipe
    return res


def ids(cases):
    return [f"{p}-{b}x{n}" for p, b, n in cases]


@pytest.mark.parametrize("case", CASES + UNGATED, ids=ids(CASES + UNGATED))
def test_two_streams_equal_one_stream(runs, case):
    assert runs[case]["two_streams"] == [True, True], case
    for name, (lo, hi) in runs[case]["selections"].items():
        if name.startswith("cnt"):                          # neighbours found: a centroid is a point of the window, and K <= 128
            assert 1 <= lo and hi <= 128, (case, name, lo, hi)
        else:                                               # indices into enc.sa1's 512 centroids / into the window
            assert 0 <= lo and hi < (512 if name == "nn1_idx" else case[2]), (case, name, lo, hi)


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_windows_alone_equal_the_same_windows_inside_a_larger_batch(runs, case):
    assert runs[case]["in_batch"], case


@pytest.mark.parametrize("how", ["eager", "graph", "inflight", "single_stream"])
@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_no_stale_reads_after_the_workspace_is_poisoned(runs, case, how):
    ok = runs[case][how]
    assert len(ok) == (2 if how == "single_stream" else ROUNDS) and all(ok), (case, how, ok)
