"""CPU: the pose-track exports' declarations and argument checks, PoseTrack's own argument checks, the output length, the yardstick of
the GPU tests (tests/ref_pose_track.py) against the fixtures the reference's interpolation wrote (tests/make_golden_pose_track.py), and
the yardstick's camera transform against its defining property on oracle/mano_oracle.py in float64."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
import torch

import ref_pose_track as RP
from ev2hands_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ["ev2h_pose_track_prepare", "ev2h_pose_track_rows", "ev2h_pose_track_hand_size"]
NAMES = ["L4", "L5", "L6", "stretch_7_4", "right_only", "edges", "long_L40"]
TOL = 1e-12                     # 200 x the 5e-15 a restatement of scipy's interpolation was measured at
SIDES = ("left", "right")


def load(name):
    fx = dict(np.load(os.path.join(GOLDEN, f"metrics_pose_track_{name}.npz")))
    fx["keys"] = tuple(fx[f"keys_{s}"] if len(fx[f"keys_{s}"]) else None for s in SIDES)
    return fx


@pytest.fixture(scope="module")
def built():
    from ev2hands_amd import build
    build.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------ the exports
def test_pose_track_exports_and_struct_are_declared_listed_and_present(built):
    hdr = open(os.path.join(ROOT, "include", "ev2hands_hip.h")).read()
    declared = set(re.findall(r"\b(ev2h_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(built, name), name
        assert getattr(built, name).argtypes is not None, f"{name} has no ctypes signature"
    assert "typedef struct ev2h_pose_track_hand" in hdr
    assert built.ev2h_pose_track_hand_size() == C.sizeof(_lib.PoseTrackHand) == 64
    assert [f[0] for f in _lib.PoseTrackHand._fields_] == ["keys", "quat", "rel", "coef", "inv_comps", "J_template", "J_shape", "n_keys", "ncomps"]
    for macro, value in (("KEY", _lib.POSE_TRACK_KEY), ("COEF", _lib.POSE_TRACK_COEF), ("PARTS", _lib.POSE_TRACK_PARTS)):
        assert re.search(rf"#define EV2H_POSE_TRACK_{macro} {value}\b", hdr), macro
    assert built.ev2h_abi_version() == 8 == _lib.ABI_VERSION
    from ev2hands_amd import build, pose_track, simulate
    assert "pose_track.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "pose_track.hip"))
    for name in ("rows", "rows64", "rows_at", "from_mano_data"):
        assert callable(getattr(pose_track.PoseTrack, name))
    assert callable(simulate.simulate_track) and callable(simulate.EventSimulatorS.step_track) and callable(simulate.EventSimulatorS.annotation_table_track)


def _hand(p, n_keys=5, K=6):
    return _lib.PoseTrackHand(p, p, p, p, p, p, p, n_keys, K)


def test_bad_arguments_return_error_codes_before_any_device_call(built):
    p = 4096                                   # stands for any non-null pointer: the argument checks come before every use
    # ev2h_pose_track_prepare(keys, n_keys, quat, rel, coef, stream)
    ok = [p, 5, p, p, p, 0]
    for i in (0, 2, 3, 4):
        assert built.ev2h_pose_track_prepare(*[0 if j == i else v for j, v in enumerate(ok)]) == 1, i
        assert b"bad argument" in built.ev2h_last_error()
    for L in (3, 0, -1, 65537):
        assert built.ev2h_pose_track_prepare(p, L, p, p, p, 0) == 1, L
    # ev2h_pose_track_rows(hands, n, f0, f1, frame_index, cam, rows_left, rows_right, ld_rows, present, parts, stream)
    def call(hands=None, n=30, f0=0, f1=30, index=0, cam=None, rl=p, rr=p, ld=22, present=p):
        hands = hands if hands is not None else (_lib.PoseTrackHand * 2)(_hand(p), _hand(p))
        return built.ev2h_pose_track_rows(hands, n, f0, f1, index, cam, rl, rr, ld, present, 0, 0)
    assert built.ev2h_pose_track_rows(None, 30, 0, 30, 0, None, p, p, 22, p, 0, 0) == 1
    for kw in (dict(n=1), dict(f0=-1), dict(f1=31), dict(f0=5, f1=5), dict(f0=6, f1=5), dict(f0=3, f1=3, index=p), dict(ld=21), dict(present=0),
               dict(rl=0), dict(rr=0)):
        assert call(**kw) == 1, kw
        assert b"bad argument" in built.ev2h_last_error()
    for h in (0, 1):
        for n_keys in (3, 1, -4, 65537):
            hands = (_lib.PoseTrackHand * 2)(_hand(p), _hand(p))
            hands[h].n_keys = n_keys
            assert call(hands) == 1, (h, n_keys)
        for K in (0, 46):
            hands = (_lib.PoseTrackHand * 2)(_hand(p), _hand(p))
            hands[h].ncomps = K
            assert call(hands, ld=64) == 1, (h, K)
        for field in ("keys", "quat", "rel", "coef", "inv_comps"):
            hands = (_lib.PoseTrackHand * 2)(_hand(p), _hand(p))
            setattr(hands[h], field, None)
            assert call(hands) == 1, (h, field)
    assert call((_lib.PoseTrackHand * 2)(_hand(p, 0), _hand(p, 0))) == 1                      # both hands absent
    cam = (C.c_double * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    cam[10] = float("nan")
    assert call(cam=cam) == 1
    cam[10] = 0.0
    hands = (_lib.PoseTrackHand * 2)(_hand(p), _hand(p))
    hands[1].J_shape = None                                                                 # the camera needs the root joint's constants
    assert call(hands, cam=cam) == 1
    assert b"bad argument" in built.ev2h_last_error()


def test_pose_track_argument_checks_raise_and_name_the_hand_and_the_row():
    from ev2hands_amd.pose_track import PoseTrack, check_arguments
    good = np.zeros((5, 61), dtype=np.float32)
    keys, n, cam = check_arguments(good, None, 5, 30)
    assert keys[1] is None and n == 30 and cam is None
    bad_row = good.copy()
    bad_row[3, 50] = np.inf
    for args, words in (((good[:3], good), ("keys_left", "3 keyframes")), ((good, good[:2]), ("keys_right", "2 keyframes")),
                        ((good, bad_row), ("keys_right", "row 3")), ((bad_row * np.float32("nan"), None), ("keys_left", "row 0")),
                        ((good.astype(np.float64), None), ("keys_left", "float32")), ((good[:, :60], None), ("keys_left", "61")),
                        ((good, good.reshape(-1)), ("keys_right", "61")), (([[0.0] * 61] * 5, None), ("keys_left", "float32")),
                        ((None, None), ("both hands",))):
        with pytest.raises(ValueError) as e:
            PoseTrack("cuda:0", None, *args)                     # the checks come before the device and the hands are looked at
        assert all(w in str(e.value) for w in words), (words, str(e.value))
    with pytest.raises(ValueError, match="n >= 2"):
        check_arguments(good, good, 30, 5)                       # 5 keyframes at 30 fps -> 5 fps: round(0.83) = 1 frame
    for fps in ((0, 30), (5, -1), (float("nan"), 30), (5, float("inf"))):
        with pytest.raises(ValueError, match="fps"):
            check_arguments(good, good, *fps)
    eye = np.eye(3)
    for camera in ((eye[:2], np.zeros(3)), (eye, np.zeros(2)), (eye * 2.0, np.zeros(3)), (np.diag([1.0, 1.0, -1.0]), np.zeros(3)),
                   (eye, np.array([0.0, np.nan, 0.0]))):
        with pytest.raises(ValueError, match="camera"):
            check_arguments(good, good, 5, 30, camera)
    assert check_arguments(good, good, 5, 30, (eye, [1.0, 2.0, 3.0]))[2][1].tolist() == [1.0, 2.0, 3.0]


def test_output_length_follows_numpy_round_at_halves():
    from ev2hands_amd.pose_track import output_length
    # max_keys / fps_in * fps_out = 2.5, 3.5, 4.5, 0.5, 1.5: halves go to the even neighbour
    assert [output_length(L, 2, 1) for L in (5, 7, 9, 1, 3)] == [2, 4, 4, 0, 2]
    assert output_length(4, 5, 30) == 24 and output_length(40, 5, 1000) == 8000 and output_length(7, 5, 30) == 42
    for L, fi, fo in ((5, 2, 1), (13, 4, 3), (50, 5, 1000), (6, 7, 29)):
        assert output_length(L, fi, fo) == RP.n_frames(L, fi, fo) == int(np.round(L / fi * fo))


# ---------------------------------------------------------------------------------------------------------------- the yardstick
def test_committed_fixtures_hold_the_stored_conditions():
    paths = sorted(glob.glob(os.path.join(GOLDEN, "metrics_pose_track_*.npz")))
    assert sorted(os.path.basename(p) for p in paths) == sorted(f"metrics_pose_track_{n}.npz" for n in NAMES)
    assert sum(os.path.getsize(p) for p in paths) < 400 * 1024
    lengths = {}
    for name in NAMES:
        fx = load(name)
        n, frames = int(fx["n"]), fx["frames"]
        lengths[name] = tuple(0 if k is None else len(k) for k in fx["keys"])
        assert n == RP.n_frames(max(lengths[name]), int(fx["fps_in"]), int(fx["fps_out"]))
        assert frames[0] == 0 and frames[-1] == n - 1 and (np.diff(frames) > 0).all() and fx["pose"].shape == (len(frames), 2, 48)
        assert list(fx["present"]) == [k is not None for k in fx["keys"]]
        for h, k in enumerate(fx["keys"]):
            if k is None:
                assert not fx["pose"][:, h].any() and not fx["shape"][:, h].any()
                continue
            assert k.dtype == np.float32
            # every rotation -- absolute and relative of the keyframes, and of the output -- is at most 2.8 rad
            q = RP.from_rotvec(k[:, :48].astype(np.float64).reshape(-1, 16, 3))
            assert (2 * np.arctan2(np.linalg.norm(q[..., :3], axis=-1), np.abs(q[..., 3]))).max() <= 2.8
            assert np.linalg.norm(RP.prepare(k.astype(np.float64))[1], axis=-1).max() <= 2.8
            assert np.linalg.norm(fx["pose"][:, h].reshape(-1, 16, 3), axis=-1).max() <= 2.8
    assert lengths == {"L4": (4, 4), "L5": (5, 5), "L6": (6, 6), "stretch_7_4": (7, 4), "right_only": (0, 5), "edges": (6, 6), "long_L40": (40, 40)}
    assert int(load("long_L40")["n"]) == 8000 and len(load("long_L40")["frames"]) < 100
    # the edge fixture holds what it is there for
    for k in load("edges")["keys"]:
        p = k[:, :48].reshape(6, 16, 3).astype(np.float64)
        assert not p[:, 1].any() and p[:, 2].all()
        assert np.abs(np.linalg.norm(p[:, 3], axis=1) - 1e-5).max() < 1e-11
        assert np.array_equal(p[3, 4], p[2, 4]) and abs(np.linalg.norm(p[1, 5]) - 4.0) < 1e-6
    assert np.array_equal(load("edges")["keys"][1][4], load("edges")["keys"][1][3])


@pytest.mark.parametrize("name", NAMES)
def test_yardstick_equals_the_reference_fixture(name):
    fx = load(name)
    n, frames = int(fx["n"]), fx["frames"]
    for h, k in enumerate(fx["keys"]):
        if k is None:
            continue
        pose, shape, trans = RP.interpolate(k.astype(np.float64), n, frames)
        full = RP.interpolate(k.astype(np.float64), n)                                   # the stored frames are a selection of all frames
        assert all(np.array_equal(a, b[frames]) for a, b in zip((pose, shape, trans), full))
        e_pose = np.abs(pose - fx["pose"][:, h]).max()
        e_shape = np.abs(shape - fx["shape"][:, h]).max() / max(1.0, np.abs(fx["shape"][:, h]).max())
        e_trans = np.abs(trans - fx["trans"][:, h]).max() / max(1.0, np.abs(fx["trans"][:, h]).max())
        print(f"{name} {SIDES[h]}: pose {e_pose:.2e} rad, shape {e_shape:.2e}, trans {e_trans:.2e}")
        assert e_pose <= TOL and e_shape <= TOL and e_trans <= TOL, (name, h, e_pose, e_shape, e_trans)
        # the first and the last frame are the first and the last keyframe
        k64 = k.astype(np.float64)
        first, last = RP.interpolate(k64, n, np.array([0, n - 1]))[0]
        q = lambda v: RP.from_rotvec(v.reshape(16, 3))
        for got, key in ((first, k64[0, :48]), (last, k64[-1, :48])):
            assert np.abs(RP.as_rotvec(RP.quat_mul(RP.conj(q(key)), q(got)))).max() <= TOL          # the same rotation (a 4.0 key comes back as 2 pi - 4)


def test_spline_is_one_cubic_at_four_keys_and_interpolates_its_knots():
    rs = np.random.RandomState(5)
    y = rs.normal(0, 1, (4, 3))
    M = RP.second_derivatives(y)
    assert np.abs(np.diff(M, 2, axis=0)).max() <= 1e-13                                   # a linear second derivative: one cubic
    for c in range(3):
        poly = np.polyfit(np.arange(4.0), y[:, c], 3)
        assert np.abs(2 * poly[1] + 6 * poly[0] * np.arange(4.0) - M[:, c]).max() <= 1e-11
    for L in (5, 6, 9, 40):
        y = rs.normal(0, 1, (L, 2))
        M = RP.second_derivatives(y)
        d = 6.0 * (y[:-2] - 2.0 * y[1:-1] + y[2:])
        assert np.abs(M[:-2] + 4.0 * M[1:-1] + M[2:] - d).max() <= 1e-12                  # C2 at every interior knot
        assert np.abs((M[1] - M[0]) - (M[2] - M[1])).max() <= 1e-12 and np.abs((M[-1] - M[-2]) - (M[-2] - M[-3])).max() <= 1e-12      # not-a-knot


# ---------------------------------------------------------------------------------------------------------------- the camera
def _rotation(rotvec):
    v = np.asarray(rotvec, dtype=np.float64)
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * Kx @ Kx


def _cameras():
    rs = np.random.RandomState(11)
    axis = np.array([0.6, 0.0, 0.8])
    rotvecs = [rs.normal(0, 1.0, 3), rs.normal(0, 2.0, 3), np.zeros(3), axis * (np.pi - 1e-9), np.array([0.0, 1e-7, 0.0]), np.array([-2.0, 1.5, 0.7])]
    return [(_rotation(v), rs.uniform(-300, 300, 3)) for v in rotvecs]


@pytest.mark.parametrize("K", [6, 45])
def test_yardstick_camera_transform_turns_the_layers_output_rigidly(K):
    from oracle import mano_oracle
    assets = {s: synth.synth_mano_surface_assets(s, 0) for s in SIDES}
    hands = mano_oracle.make_hands(assets["left"], assets["right"], K, dtype=torch.float64)
    fx = load("stretch_7_4")
    invs = [RP.inverse_components(assets[s]["hands_components"]) for s in SIDES]
    roots = []
    for s in SIDES:                                           # the rest root joint's constant and shape terms, in the oracle's own float64
        o = hands[s]
        jr, vt, sd = o.J_regressor.numpy(), o.v_template[0].numpy(), o.shapedirs.numpy()
        roots.append(((jr @ vt)[0], np.einsum("v,vck->kc", jr[0], sd)))
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    worst = 0.0
    for R, t_mm in _cameras():
        out = RP.track(fx["keys"], 5, 30, invs, K, camera_rt=(R, t_mm), roots=roots)
        for h, s in enumerate(SIDES):
            pca, betas = out["pca"][:, h, :K], out["shape"][:, h]
            before = hands[s](t64(out["pose"][:, h, :3]), t64(pca), t64(betas), t64(out["trans"][:, h]))
            after = hands[s](t64(out["global_orient"][:, h]), t64(pca), t64(betas), t64(out["transl"][:, h]))
            for a, b in ((after.vertices, before.vertices), (after.joints, before.joints)):
                want = b.numpy() @ R.T + t_mm / 1000.0
                worst = max(worst, np.abs(a.numpy() - want).max())
    print(f"K = {K}: max |layer(transformed rows) - (R layer(rows) + t)| = {worst:.2e} m")
    assert worst <= 1e-9
    # the identity camera leaves the rows as they are, but for the roundings of log(exp(.)) and of + J0 - J0 (values below 2)
    out = RP.track(fx["keys"], 5, 30, invs, K, camera_rt=(np.eye(3), np.zeros(3)), roots=roots)
    assert np.abs(out["global_orient"] - out["pose"][:, :, :3]).max() <= 1e-15 and np.abs(out["transl"] - out["trans"]).max() <= 1e-15


def test_pca_product_undoes_the_components_and_keys_follow_upstreams_gathering():
    assets = synth.synth_mano_surface_assets("right", 0)
    inv = RP.inverse_components(assets["hands_components"])
    rs = np.random.RandomState(2)
    coef = rs.normal(0, 1, (7, 45))
    pose = np.concatenate([np.zeros((7, 3)), coef @ np.asarray(assets["hands_components"], dtype=np.float64)], 1)
    got, bound = RP.pca(pose, inv)
    assert np.abs(got - coef).max() <= 1e-4 * bound.max()                                  # a float32 inverse
    assert np.abs(got - pose[:, 3:] @ inv).max() <= 1e-12 * (1 + bound.max())
    # a hand that is None in a keyframe is skipped; frames are ordered by int(key); a hand that never has data is absent
    row = lambda v: {"pose": [v] * 48, "shape": [v] * 10, "trans": [v] * 3}
    data = {"10": {"left": row(2.0), "right": None}, "9": {"left": row(1.0), "right": row(5.0)}, "100": {"left": row(3.0), "right": row(6.0)}}
    left, right = RP.keys_from_mano_data(data)
    assert left[:, 0].tolist() == [1.0, 2.0, 3.0] and right[:, 0].tolist() == [5.0, 6.0] and left.dtype == np.float32 and left.shape == (3, 61)
    assert RP.keys_from_mano_data({"1": {"left": None, "right": row(1.0)}})[0] is None
