"""GPU: the augmented Ev2Hands-S training item on the device (csrc/events.hip: ev2h_event_window_build_s_ranges_aug;
EventWindowBuilderS.accumulate_ranges(noise= / augment=); ev2hands_amd/train_data.py: TrainingBatcherS).

Nothing here compares the new code with itself: the explicit path is held to what the reference's Ev2HandSDataset.__getitem__
returned with augment on (tests/golden/events_augment_s_*.npz) and, at the hand-made edges, to the NumPy restatement tests/ref_augment.py
(pinned to the reference by tests/make_golden_augment.py and tests/test_augment_cpu.py); the seeded path to the same restatement
fed with the draws of tests/ref_philox.py; the un-augmented calls to the parent's route."""
import os

import numpy as np
import pytest
import torch

import ref_augment as RA
import ref_evaluate_s as RS
import ref_philox as RP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x9E3779B97F4A7C15
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NO_WINDOW = 2 ** 31 - 1


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(DEV, dtype) if dtype is not None else t.to(DEV)


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _noise_batch(noises):
    """[None | float64 [K, 5]] -> (rows [B, Kmax, 5] float64 filled with NaN beyond a window's rows, n [B] int32, -1 for None)"""
    kmax = max([1] + [n.shape[0] for n in noises if n is not None])
    rows = np.full((len(noises), kmax, 5), np.nan)
    n = np.full(len(noises), -1, dtype=np.int32)
    for b, z in enumerate(noises):
        if z is not None:
            rows[b, :z.shape[0]], n[b] = z, z.shape[0]
    return rows, n


def _check_window(got, b, want_table, want_lab, name=""):
    """window b of accumulate_ranges' outputs against a restated / recorded sorted table"""
    sorted_t, counts, labels, _ = got
    T = want_table.shape[0]
    assert int(counts[b]) == T, (name, int(counts[b]), T)
    st = _np(sorted_t[b, :T])
    assert np.array_equal(_bits(st[:, :5]), _bits(want_table)), name
    assert not st[:, 5:].any(), name
    assert np.array_equal(_np(labels[b, :T]), want_lab), name


# ------------------------------------------------------------------------------------------------ 1. explicit noise, the fixtures
def test_explicit_path_equals_the_references_items_on_every_fixture():
    _need_gpu()
    from ev2hands_amd.events import EventTableS, EventWindowBuilderS
    fx = RA.load_fixtures(GOLDEN)
    assert len(fx) == 9
    bld = EventWindowBuilderS(DEV)
    # the two full windows share a table and a call: one augmented, one not (noise_n = -1)
    groups = [([fx[0], fx[1]], np.concatenate([fx[0][1]["rows"], fx[1][1]["rows"]]), [0, 2048])] + [([f], f[1]["rows"], [0]) for f in fx[2:]]
    for wins, rows, starts in groups:
        table = EventTableS(DEV, rows)
        noises = [w["noise"] if int(w["coin"]) else None for _, w in wins]
        coin = torch.full((len(wins),), 7, dtype=torch.int32, device=DEV)
        got = bld.accumulate_ranges(table, _i32(starts), noise=_noise_batch(noises), coin=coin)
        assert list(_np(coin)) == [int(w["coin"]) for _, w in wins]
        for b, (name, w) in enumerate(wins):
            _check_window(got, b, w["table"], w["table_lab"], name)
        idx = np.stack([w["idx"] for _, w in wins])
        ev, lab = bld.sample(got[0], got[1], idx, got[2])
        for b, (name, w) in enumerate(wins):
            assert np.array_equal(_bits(_np(ev[b])), _bits(w["events"])), name
            assert lab.dtype == torch.int64 and np.array_equal(_np(lab[b]), w["labels"]), name


# ------------------------------------------------------------------------------------- 2. not augmented: today's outputs, bit for bit
def test_unaugmented_calls_give_todays_outputs():
    _need_gpu()
    from ev2hands_amd.events import EventTableS, EventWindowBuilderS
    fx = RA.load_fixtures(GOLDEN)
    rows = np.concatenate([fx[0][1]["rows"], fx[1][1]["rows"]])
    E = rows.shape[0]
    starts = [0, 700, 2048, E - 600, E - 10]
    table, bld = EventTableS(DEV, rows), EventWindowBuilderS(DEV)
    st = _i32(starts)
    # the parent's route: windows cut on the host, built and sorted by __call__ (ev2h_event_window_build + ev2h_event_window_timesort)
    host = EventWindowBuilderS(DEV)
    host([rows[s:s + 2048] for s in starts], sample_idx=np.zeros((len(starts), 2048), dtype=np.int64))
    ht, hl = _np(host.table), _np(host.table_labels)
    plain = bld.accumulate_ranges(table, st)
    off = bld.accumulate_ranges(table, st, noise=(np.zeros((len(starts), 1, 5)), np.full(len(starts), -1, dtype=np.int32)))
    ms = _np(plain[1])
    assert (ms > 0).all() and np.array_equal(ms, _np(off[1]))
    for b, m in enumerate(ms):
        for got in (plain, off):
            assert np.array_equal(_bits(_np(got[0][b, :m])), _bits(ht[b, :m])), b
            assert np.array_equal(_np(got[2][b, :m]), hl[b, :m]) and not _np(got[2][b, m:]).any(), b
    assert torch.equal(plain[3], off[3])
    # window 2 is the fixture the reference built with the coin down
    _check_window(plain, 2, fx[1][1]["table"], fx[1][1]["table_lab"])
    # both sources, a coin without a source, a table beyond the sort's reach, window ids on the host: refused before any launch
    ids = _i32(range(len(starts)))
    with pytest.raises(ValueError):
        bld.accumulate_ranges(table, st, noise=(np.zeros((len(starts), 1, 5)), np.zeros(len(starts), dtype=np.int32)), augment=(1, ids))
    with pytest.raises(ValueError):
        bld.accumulate_ranges(table, st, coin=torch.zeros(len(starts), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        EventWindowBuilderS(DEV, cap=16384).accumulate_ranges(table, st, augment=(1, ids))
    with pytest.raises(ValueError):
        bld.accumulate_ranges(table, st, augment=(1, ids.cpu()))
    with pytest.raises(ValueError):
        bld.accumulate_ranges(table, st, noise=(np.zeros((len(starts), 1, 4)), np.zeros(len(starts), dtype=np.int32)))


# ---------------------------------------------------------------------------------------------------- 3. explicit noise, the edges
def _distinct_rows(E, seed):
    """E events on E distinct pixels, increasing nanosecond times, labels 0 .. 2, annotation 0"""
    rs = np.random.RandomState(seed)
    pix = rs.permutation(346 * 260)[:E]
    t = np.cumsum(1000.0 * (1 + rs.randint(0, 3, E)) + rs.randint(0, 1000, E)).astype(np.float64)
    return np.stack([pix % 346, pix // 346, t, rs.rand(E) < 0.5, np.zeros(E), rs.randint(0, 3, E)], 1).astype(np.float64)


def test_explicit_edges_equal_the_restatement():
    _need_gpu()
    from ev2hands_amd.events import EventTableS, EventWindowBuilderS
    N = 256
    rows = _distinct_rows(40, 3)
    pix, _ = RA.pixel_table(rows)
    M = pix.shape[0]
    assert M == 40
    early = float(pix[:, 2].min()) - 0.123456789                    # before every pixel: the time subtracted is no float32 value
    assert np.float64(np.float32(early)) != early
    tie = float(pix[17, 2])                                          # exactly a pixel's time: the pixel comes first
    noise = np.array([[5.0, 6.0, early, 1.0, 2.0], [7.0, 8.0, tie, 3.0, 0.0], [pix[3, 0], pix[3, 1], float(pix[:, 2].max()) + 731.25, 0.0, 7.0]])
    want_t, want_l, order = RA.sorted_table(rows, noise)
    assert order[0] == M and list(order).index(17) + 1 == list(order).index(M + 1) and want_t.shape[0] == M + 3
    assert (want_t[:, :2] == pix[3, :2]).all(1).sum() == 2           # the occupied pixel stays two rows
    px = order[1:] < M                                               # float32 arithmetic would give other bits in some rows
    assert (want_t[1:][px, 2] != (pix[order[1:][px], 2] - np.float32(early)).astype(np.float32)).any()
    table = EventTableS(DEV, rows)
    bld = EventWindowBuilderS(DEV, n_events=N)
    # [the window, an empty one (start outside the table), the window without noise rows, the window not augmented]
    noises = [noise, noise, np.zeros((0, 5)), None]
    got = bld.accumulate_ranges(table, _i32([0, -1, 0, 0]), noise=_noise_batch(noises))
    assert list(_np(got[1])) == [M + 3, 0, M, M] and list(_np(got[3])) == [0, -1, 0, 0]
    _check_window(got, 0, want_t, want_l, "three noise rows")
    plain_t, plain_l, _ = RA.sorted_table(rows, None)
    _check_window(got, 2, *RA.sorted_table(rows, np.zeros((0, 5)))[:2], "K = 0")
    _check_window(got, 3, plain_t, plain_l, "not augmented")
    idx = np.random.RandomState(5).randint(0, M + 3, N)
    ev, lab = bld.sample(got[0][:1], got[1][:1], idx[None], got[2][:1])
    want_ev, want_lab, _, _ = RA.item(rows, noise, idx)
    assert np.array_equal(_bits(_np(ev[0])), _bits(want_ev)) and np.array_equal(_np(lab[0]), want_lab)
    # the empty window is refused by the seeded sampler, by name, and the others are drawn
    status = torch.full((1,), NO_WINDOW, dtype=torch.int32, device=DEV)
    bld.sample_seeded(got[0], got[1], SEED, _i32([10, 11, 12, 13]), labels=got[2], status=status)
    assert int(status) == 11

    # cap: M + K == cap is built, M + K == cap + 1 gets its count and no table
    small = EventWindowBuilderS(DEV, n_events=N, cap=64)
    rows61 = _distinct_rows(61, 4)
    p61, _ = RA.pixel_table(rows61)
    rs = np.random.RandomState(6)
    z4 = np.stack([rs.randint(0, 346, 4), rs.randint(0, 260, 4), p61[rs.randint(0, 60, 4), 2].astype(np.float64) + rs.rand(4) * 1e3,
                   rs.randint(0, 9, 4), rs.randint(0, 9, 4)], 1).astype(np.float64)
    t61 = EventTableS(DEV, rows61)
    out = (torch.full((2, 64, 8), -5.0, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV), torch.full((2, 64), -5, dtype=torch.int32, device=DEV),
           torch.zeros(2, dtype=torch.int32, device=DEV))
    got = small.accumulate_ranges(t61, _i32([0, 0]), out=out, noise=_noise_batch([z4[:3], z4]))
    assert got[0] is out[0] and list(_np(got[1])) == [64, 65]
    _check_window(got, 0, *RA.sorted_table(rows61, z4[:3])[:2], "M + K == cap")
    assert (_np(out[0][1]) == -5.0).all() and (_np(out[2][1]) == -5).all()           # refused: nothing written
    status = torch.full((1,), NO_WINDOW, dtype=torch.int32, device=DEV)
    ev = small.sample_seeded(got[0], got[1], SEED, _i32([20, 21]), status=status)
    assert int(status) == 21 and not _np(ev[1]).any() and _np(ev[0]).any()


# ------------------------------------------------------------------------------------------------------------ 4. the seeded path
E_ROWS = 6000


def _ids_with_both_coins():
    """five window ids, neither consecutive nor in order: the coin up for windows 0, 2 and 3, down for 1 and 4"""
    up = [k for k in range(1000, 1100) if RA.coin(SEED, k)]
    down = [k for k in range(50, 150) if not RA.coin(SEED, k)]
    ids = [up[0], down[0], up[1], 2 ** 31 - 1 if RA.coin(SEED, 2 ** 31 - 1) else up[2], down[1]]
    return ids, [RA.coin(SEED, k) for k in ids]


@pytest.mark.parametrize("n_events", [256, 2048])
def test_seeded_path_equals_the_restatement_and_does_not_depend_on_the_batch(n_events):
    _need_gpu()
    from ev2hands_amd.events import EventTableS, EventWindowBuilderS
    rows = RS.synth_table(E_ROWS, 17)
    starts = [0, 1311, 2500, E_ROWS - n_events - 1, E_ROWS - 10]     # the last window has 10 rows: K = 0 whatever the coin
    ids, coins = _ids_with_both_coins()
    assert coins == [True, False, True, True, False]
    table, bld = EventTableS(DEV, rows), EventWindowBuilderS(DEV, n_events=n_events)
    coin = torch.zeros(len(starts), dtype=torch.int32, device=DEV)
    st, wid = _i32(starts), _i32(ids)
    got = bld.accumulate_ranges(table, st, augment=(SEED, wid), coin=coin)
    ev, lab, idx = bld.sample_seeded(got[0], got[1], SEED, wid, labels=got[2], return_idx=True)
    assert list(_np(coin)) == [int(c) for c in coins]
    ks = []
    for b, (s, k) in enumerate(zip(starts, ids)):
        window = rows[s:s + n_events]
        want_ev, want_lab, want_t, want_tl, aug = RA.seeded_item(window, SEED, k, n_events)
        assert aug == coins[b]
        _check_window(got, b, want_t, want_tl, f"window {b}")
        M = RA.pixel_table(window)[0].shape[0]
        ks.append(want_t.shape[0] - M)
        assert ks[-1] == (M // 32 if aug else 0)
        assert np.array_equal(_np(idx[b]), RP.sample_indices(SEED, k, want_t.shape[0], n_events)), b
        assert np.array_equal(_bits(_np(ev[b])), _bits(want_ev)) and np.array_equal(_np(lab[b]), want_lab), b
        assert int(got[3][b]) == int(window[-1, 4])
    assert max(ks) >= 2 and ks[-1] == 0
    # each window alone, and two shards with their true ids: the same bits
    for sl in [slice(b, b + 1) for b in range(len(starts))] + [slice(0, 2), slice(2, 5)]:
        part = bld.accumulate_ranges(table, st[sl].contiguous(), augment=(SEED, wid[sl].contiguous()))
        pe, pl = bld.sample_seeded(part[0], part[1], SEED, wid[sl].contiguous(), labels=part[2])
        assert torch.equal(part[1], got[1][sl]) and torch.equal(part[3], got[3][sl])
        for b in range(sl.start, sl.stop):
            T = int(got[1][b])
            assert torch.equal(part[0][b - sl.start, :T].view(torch.int32), got[0][b, :T].view(torch.int32)), b
            assert torch.equal(part[2][b - sl.start, :T], got[2][b, :T]), b
        assert torch.equal(pe.view(torch.int32), ev[sl].view(torch.int32)) and torch.equal(pl, lab[sl])
    # another id is another item
    other = bld.accumulate_ranges(table, st, augment=(SEED, wid + 1))
    assert not torch.equal(other[0][:, :200], got[0][:, :200])


# --------------------------------------------------------------------------------------------------------------- 5. the batcher
def _make_net():
    from ev2hands_amd import synth
    from ev2hands_amd.model import TEHNetWrapper
    os.environ["ERPC"] = "1"
    assets = {s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")}
    net = TEHNetWrapper(DEV, mano_assets=assets, precision="f16x2")
    net.load_state_dict(synth.synth_state_dict(5, 0), strict=True)
    net.eval()
    return net


def _annotations(A=3):
    from ev2hands_amd import synth
    out = {}
    for a in range(A):
        hands = {}
        for side in ("left", "right"):
            tag = f"train-batch/{a}/{side}"
            hands[side] = {"global_orient": synth.hash_normal(tag + "/go", (1, 3), 7) * 0.3, "hand_pose": synth.hash_normal(tag + "/hp", (1, 45), 7) * 0.4,
                           "shape": synth.hash_normal(tag + "/sh", (1, 10), 7) * 0.5,
                           "trans": synth.hash_normal(tag + "/tr", (1, 3), 7) * 0.05 + np.array([[0.1 if side == "right" else -0.1, 0.0, 0.5]])}
        out[a] = hands
    del out[1]["left"]                                             # a missing hand: the right one's parameters stand in
    return out


def test_training_batcher_gives_the_collated_batch_and_feeds_the_loss():
    _need_gpu()
    from ev2hands_amd.evaluate import annotation_flags, annotation_table
    from ev2hands_amd.events import EventTableS, EventWindowBuilderS
    from ev2hands_amd.losses import Loss
    from ev2hands_amd.train_data import TrainingBatcherS
    N, B, K = 256, 3, 6
    rows = RS.synth_table(E_ROWS, 17)
    starts = [100, 2900, 5000]                                     # annotation indices 0, 1 (no left hand) and 2
    ids = [k for k in range(40) if RA.coin(SEED, k)][:2] + [k for k in range(40) if not RA.coin(SEED, k)][:1]
    annotations = _annotations()
    table = EventTableS(DEV, rows)
    st, wid = _i32(starts), _i32(ids)
    batcher = TrainingBatcherS(DEV, annotations, seed=SEED, batch=4, n_events=N)
    with pytest.raises(RuntimeError):
        batcher.batch(st, wid)                                     # before begin
    batcher.begin(table)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                        # device work only
    try:
        batch = batcher.batch(st, wid)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    batcher.check()
    hand_keys = ["global_orient", "hand_pose", "shape", "trans", "valid"]
    assert list(batch) == ["events", "class_logits", "mano_gt", "handedness", "left", "right", "augmented"]
    spec = {"events": ((B, 5, N), torch.float32), "class_logits": ((B, N), torch.int64), "mano_gt": ((B,), torch.float64),
            "handedness": ((B, 2), torch.int32), "augmented": ((B,), torch.bool)}
    for k, (shape, dt) in spec.items():
        assert tuple(batch[k].shape) == shape and batch[k].dtype == dt and batch[k].device == torch.device(DEV), k
    hand_spec = {"global_orient": (B, 3), "hand_pose": (B, K), "shape": (B, 10), "trans": (B, 3), "valid": (B,)}
    for side in ("left", "right"):
        assert list(batch[side]) == hand_keys
        for k, shape in hand_spec.items():
            assert tuple(batch[side][k].shape) == shape and batch[side][k].dtype == (torch.bool if k == "valid" else torch.float32), (side, k)
    # the pieces, assembled by hand
    bld = EventWindowBuilderS(DEV, n_events=N)
    got = bld.accumulate_ranges(table, st, augment=(SEED, wid))
    ev, lab = bld.sample_seeded(got[0], got[1], SEED, wid, labels=got[2])
    anno = [int(rows[min(s + N, E_ROWS) - 1, 4]) for s in starts]
    assert anno == [0, 1, 2] and list(_np(got[3])) == anno
    prm, flg = annotation_table(annotations, K)[anno], annotation_flags(annotations)[anno]
    hand = {"events": ev, "class_logits": lab, "mano_gt": torch.ones(B, dtype=torch.float64, device=DEV), "handedness": _dev(flg[:, :, 1])}
    for h, side in enumerate(("left", "right")):
        hand[side] = {"global_orient": _dev(prm[:, h, :3]), "hand_pose": _dev(prm[:, h, 3:3 + K]), "shape": _dev(prm[:, h, 3 + K:13 + K]),
                      "trans": _dev(prm[:, h, 13 + K:]), "valid": _dev(flg[:, h, 0] != 0)}
    assert torch.equal(batch["events"].view(torch.int32), ev.view(torch.int32)) and torch.equal(batch["class_logits"], lab)
    assert _np(batch["mano_gt"]).tolist() == [1.0] * B and list(_np(batch["augmented"])) == [True, True, False]
    assert np.array_equal(_np(batch["handedness"]), [[1, 1], [0, 1], [1, 1]])
    assert list(_np(batch["left"]["valid"])) == [True, False, True] == list(_np(batch["right"]["valid"]))      # upstream's shared dict
    for side in ("left", "right"):
        for k in hand_keys:
            assert torch.equal(batch[side][k], hand[side][k]), (side, k)
    assert torch.equal(batch["left"]["shape"][1], batch["right"]["shape"][1])          # the missing hand takes the other's parameters
    # each window's item is the restatement's, so the batch is the reference's recipe on the project's draws
    for b, (s, k) in enumerate(zip(starts, ids)):
        want_ev, want_lab, _, _, aug = RA.seeded_item(rows[s:s + N], SEED, k, N)
        assert np.array_equal(_bits(_np(batch["events"][b])), _bits(want_ev)) and np.array_equal(_np(batch["class_logits"][b]), want_lab), b
    # into the network and the loss
    net = _make_net()
    loss = Loss(net.hands, DEV)
    with torch.no_grad():
        outs = net(batch["events"][:, :net.net.in_channels].contiguous())
    got_loss, want_loss = loss(outs, batch), loss(outs, hand)
    assert list(got_loss) == list(want_loss) and "loss_class_logits" in got_loss
    for k in want_loss:
        assert torch.equal(got_loss[k].view(torch.int32), want_loss[k].view(torch.int32)) and bool(torch.isfinite(got_loss[k])), k
    # augment=False: the validation loader's items -- the plain table, the same draws of stream 0
    val = TrainingBatcherS(DEV, annotations, seed=SEED, batch=B, n_events=N, augment=False)
    val.begin(table)
    vb = val.batch(st, wid)
    plain = bld.accumulate_ranges(table, st)
    pe, pl = bld.sample_seeded(plain[0], plain[1], SEED, wid, labels=plain[2])
    assert torch.equal(vb["events"].view(torch.int32), pe.view(torch.int32)) and torch.equal(vb["class_logits"], pl) and not _np(vb["augmented"]).any()
    assert not torch.equal(vb["events"][0], batch["events"][0])
    # a window that cannot be built is named by check(); more windows than `batch` are refused
    bad = batcher.batch(_i32([100, E_ROWS, 5000]), wid)
    assert not _np(bad["events"][1]).any()
    with pytest.raises(RuntimeError, match=f"window {ids[1]}"):
        batcher.check()
    with pytest.raises(ValueError):
        batcher.batch(_i32([0] * 5), _i32(range(5)))
    with pytest.raises(ValueError):
        batcher.batch(st.long(), wid)
