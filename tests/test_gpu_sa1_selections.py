"""GPU: the two chunked schedules of enc.sa1's selections (forward.hip) against the one-launch schedule (EV2H_FPS_CHUNKS=0), bit for
bit -- from 8 windows on, the sampling in four chunks on the side stream and the ball query of each quarter on the caller's; from 64
windows of at most 2048 points on, one-job sampling chunks each followed by its quarter's ball query on the side stream, and the
regressors' samplings behind them -- and against stale reads: a consumer that misses an event edge reads what the LAST forward left
in the workspace, which is invisible while every forward sees the same input -- so the inputs alternate and the whole workspace is
overwritten with 0xFF bytes between two forwards.

EV2H_FPS_CHUNKS is read once per process: each schedule runs in a child process of its own (started with subprocess, under its own
timeout; after a child that failed nothing more is started).  Both children compute everything once; the tests compare what they saved.

Shapes: 8 windows (the smallest batch the chunked path takes) and 9 (a multiple of nothing), 64 (the smallest batch whose queries run
on the side stream) and 65, 512 points (fps_kernel<2>, N equal to enc.sa1's 512 centroids) and 2048; f16x2, and bf16 once per schedule."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [("f16x2", 8, 512), ("f16x2", 9, 512), ("f16x2", 8, 2048), ("f16x2", 9, 2048), ("bf16", 9, 2048),
         ("f16x2", 64, 512), ("f16x2", 65, 2048), ("bf16", 65, 2048)]
REGIONS = ("fps1", "fpsmL", "fpsmR", "gidx1_0", "gidx1_1", "gidx1_2", "cnt1")
ROUNDS = 5

_CHILD = """
import os, sys, torch
sys.path.insert(0, {root!r})
from ev2hands_amd import _lib, synth
from ev2hands_amd.inflight import InflightForward
from ev2hands_amd.model import TEHNetWrapper
os.environ['ERPC'] = '0'
CASES, REGIONS, ROUNDS, stale = {cases!r}, {regions!r}, {rounds!r}, sys.argv[2] == 'stale'
assets = {{s: synth.synth_mano_assets(s, 4) for s in ('left', 'right')}}
sd = synth.synth_state_dict(4, 4)


def make(prec):
    net = TEHNetWrapper('cuda:0', mano_assets=assets, precision=prec)
    net.load_state_dict(sd, strict=True); net.eval()
    return net


def flat(o):
    return {{'class_logits': o['class_logits'].clone(),
             **{{f'{{s}}.{{k}}': o[s][k].clone() for s in ('left', 'right') for k in ('vertices', 'j3d', 'global_orient', 'hand_pose', 'betas', 'transl')}}}}


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in b)


res = {{}}
nets = {{}}
for prec, B, N in CASES:
    net = nets.get(prec) or nets.setdefault(prec, make(prec))
    inp = [(synth.synth_cloud('E', B, 4, N, 11 + i).cuda(), synth.fps_inits(B, N, 11 + i)) for i in range(2)]       # X, Y

    def fwd(i, n=net):
        n.net.fps_init = inp[i][1]
        with torch.no_grad():
            o = flat(n(inp[i][0]))
        torch.cuda.synchronize()
        return o

    r = res[(prec, B, N)] = {{'out': [], 'ws': []}}
    for i in range(2):
        fresh = make(prec)                                      # a fresh model (its own workspace) per input
        r['out'].append({{k: v.cpu() for k, v in fwd(i, fresh).items()}})
        regions = {{name: fresh.net.debug_buffer(name, torch.int32) for name in REGIONS}}
        assert all(0 <= int(v.min()) and int(v.max()) < 32768 for v in regions.values())       # indices and counts: int16 holds them exactly
        r['ws'].append({{name: v.to(torch.int16).cpu() for name, v in regions.items()}})
    if not stale:
        continue
    want = [{{k: v.cuda() for k, v in o.items()}} for o in r['out']]
    # eager: forward, poison the whole workspace, forward on the other input
    fwd(0)
    ok = []
    for k in range(ROUNDS):
        net.net._ws.fill_(0xFF)
        ok.append(same(fwd((k + 1) & 1), want[(k + 1) & 1]))
    r['eager'] = ok
    # single-stream mode
    prev = _lib.lib().ev2h_set_side_stream(0)
    net.net._ws.fill_(0xFF)
    r['single_stream'] = [same(fwd(i), want[i]) for i in range(2)]
    _lib.lib().ev2h_set_side_stream(prev)
    # hipGraph: captured once, replayed on refreshed static inputs
    g = net.net.capture(inp[0][0], net.hands, inp[0][1])
    ok = []
    for k in range(ROUNDS):
        torch.cuda.synchronize()
        g._ws.fill_(0xFF)
        o = g.replay(inp[(k + 1) & 1][0], inp[(k + 1) & 1][1])
        torch.cuda.synchronize()
        ok.append(same(flat(o), want[(k + 1) & 1]))
    r['graph'] = ok
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
        pipe.drain(); torch.cuda.synchronize()
        if k:                                                   # (round 0 fills the slots' workspaces with real values to go stale)
            ok.append(all(same(o, want[i]) for o, i in zip(outs, order)))
        for w in pipe.ws:
            w.fill_(0xFF)
    r['inflight'] = ok
    del pipe
torch.save(res, sys.argv[1])
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = tmp_path_factory.mktemp("sa1_selections")
    script = d / "run.py"
    script.write_text(_CHILD.format(root=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), cases=CASES, regions=REGIONS, rounds=ROUNDS))
    env0 = {k: v for k, v in os.environ.items() if k not in ("EV2H_FPS_CHUNKS", "EV2H_TWO_STREAMS", "EV2H_L1_TABLE")}
    out = {}
    for tag, env, mode in (("chunked", {}, "stale"), ("one_launch", {"EV2H_FPS_CHUNKS": "0"}, "plain")):
        r = subprocess.run([sys.executable, str(script), str(d / f"{tag}.pt"), mode], env=dict(env0, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (tag, r.returncode, r.stderr[-2000:])         # (raises: a later child is never started)
        out[tag] = torch.load(d / f"{tag}.pt")
    return out


IDS = [f"{p}-{b}x{n}" for p, b, n in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_chunked_schedule_equals_one_launch(runs, case):
    a, b = runs["chunked"][case], runs["one_launch"][case]
    for i in range(2):
        for k, w in b["out"][i].items():
            assert torch.equal(a["out"][i][k], w), (case, i, k)
        for name in REGIONS:
            assert torch.equal(a["ws"][i][name], b["ws"][i][name]), (case, i, name)
        # the selections are real ones (not two equal poisoned buffers): every sampled index is a point of the window
        for name in ("fps1", "fpsmL", "fpsmR"):
            assert int(b["ws"][i][name].min()) >= 0 and int(b["ws"][i][name].max()) < case[2], (case, i, name)


@pytest.mark.parametrize("how", ["eager", "graph", "inflight", "single_stream"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_no_stale_reads_after_the_workspace_is_poisoned(runs, case, how):
    """Every forward that follows a poisoned workspace equals the fresh model's forward on the same input (saved by the same child;
    test_chunked_schedule_equals_one_launch ties that one to the one-launch schedule)."""
    ok = runs["chunked"][case][how]
    assert len(ok) == (2 if how == "single_stream" else ROUNDS) and all(ok), (case, how, ok)
