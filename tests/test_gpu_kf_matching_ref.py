"""GPU: the KeyFrame-side matchers against tests/ref_kf_matching.py.

k_bow_match<false / true>, k_tri_match, k_fuse<false / true> and k_sim3_match + k_sim3_resolve
are held to the independent NumPy statement of the reference on the scenes of
kf_matching_scenes.py (every output array and count equal, after the margin filter): through
the ORBmatcher host entries scene by scene, through each batched device entry with pairs of
different counts in one launch (an empty KeyFrame, an empty point list, rows past a count left
untouched), and at the capacities where the grid in LDS crosses 64 KiB: (3072 + 4) * 4 + 12 *
cap > 65536 from cap = 4437 on, where launch_fuse and launch_search_by_sim3 opt in to more
dynamic LDS, up to 8192; past it, and past 4096 for the BoW entries, ORBG_ENOTSUP with the
outputs untouched.  Nothing here reads the oracle.

Kernel-level sharpness, checked once on an MI355X with scratch builds (not committed).  With
`best1 <= BM_TH_LOW` in the KFKF branch of k_bow_match exactly the scenes built for that rule
fail: test_kernels_equal_reference[bowkf_thresholds50] and [bowkf_thresholds75] (a best
distance of exactly 50), and with them the two generated bowkf_random scenes; every bow_* and
every other bowkf_* test passes.  With `(unsigned)(0xFFFF - pos)` in tri_key's low bits (the
first instead of the last of the least distance; the position was decoded the same way where
the winner is read back, so that the mutant reads no index past its node) they are
[tri_ties] and [tri_second] (ties across and inside the 64-chunks), [tri_geometry] and
[tri_geometry_only_stereo] (a later equal distance wins) and test_fv_batch_device[tri], which
runs those scenes; everything else passes.

Measured on an MI355X: every scene and every batch call equal.
"""
import ctypes as C

import numpy as np
import pytest

import kf_matching_scenes as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_kernels_equal_reference(name):
    s = S.scene(name)
    S.check_equal(S.run_gpu(s), s, name)


# ---------------------------------------------------------------- device packing
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _fill(n, value=-9):
    import torch
    return torch.full((n,), value, dtype=torch.int32, device="cuda")


EMPTY_FV = (np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32))
EMPTY_SIDE = dict(kps=np.zeros(0, S.KP_DTYPE), desc=np.zeros((0, 32), np.uint8),
                  ok=np.zeros(0, np.uint8), uright=np.zeros(0, np.float32), fv=EMPTY_FV)


def _pack(sides, cap, flag_of=lambda s: s["ok"]):
    """KeyFrames of different counts at the front of their cap-sized slots."""
    from orb_slam2_test_amd import _lib as L
    nk = len(sides)
    a = dict(desc=np.zeros((nk, cap, 32), np.uint8), kps=np.zeros((nk, cap), L.KP_DTYPE),
             ur=np.full((nk, cap), -1.0, np.float32), flag=np.zeros((nk, cap), np.uint8),
             cnt=np.zeros(nk, np.int32), nodes=np.zeros((nk, cap), np.int32),
             off=np.zeros((nk, cap + 1), np.int32), feats=np.zeros((nk, cap), np.int32),
             nfv=np.zeros(nk, np.int32))
    for k, s in enumerate(sides):
        n = len(s["kps"])
        assert n <= cap
        a["desc"][k, :n], a["kps"][k, :n], a["cnt"][k] = s["desc"], s["kps"], n
        if s.get("uright") is not None:
            a["ur"][k, :n] = s["uright"]
        if s.get("ok") is not None:
            a["flag"][k, :n] = flag_of(s)
        fn, fo, ff = s.get("fv", EMPTY_FV)
        a["nodes"][k, :len(fn)], a["off"][k, :len(fo)], a["feats"][k, :len(ff)] = fn, fo, ff
        a["nfv"][k] = len(fn)
    return {k: _dev(v) for k, v in a.items()}


def _ctx():
    from orb_slam2_test_amd.orbmatcher import _ctx as ctx
    return ctx()


def _sync():
    import torch
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the FeatureVector entries
def fv_batch(kind, scenes, cap, expect_rc=0):
    """One launch over the scenes' pairs: KeyFrame 2p is the walked side of scene p, 2p + 1
    its candidate side.  Returns (match[P, cap], n[P])."""
    from orb_slam2_test_amd import _lib as L
    sides = [s[k] for s in scenes for k in ("s1", "s2")]
    P = len(scenes)
    ctx = _ctx()
    i1 = _dev(np.arange(0, 2 * P, 2, dtype=np.int32))
    i2 = _dev(np.arange(1, 2 * P, 2, dtype=np.int32))
    dm, dn = _fill(P * cap), _fill(P)
    lib = L.lib()
    if kind == "tri":
        t = _pack(sides, cap, lambda s: 1 - s["ok"])
        K = L.KeyFrames(t["desc"].data_ptr(), t["kps"].data_ptr(), t["ur"].data_ptr(),
                        t["flag"].data_ptr(), t["cnt"].data_ptr(), t["nodes"].data_ptr(),
                        t["off"].data_ptr(), t["feats"].data_ptr(), t["nfv"].data_ptr())
        G = np.zeros(P, L.TRI_GEOM_DTYPE)
        for p, s in enumerate(scenes):
            G[p] = s["geom"]
        dg = _dev(G)
        _sync()
        rc = lib.orbg_search_for_triangulation_batch_device(
            ctx.handle, C.byref(K), cap, i1.data_ptr(), i2.data_ptr(), dg.data_ptr(), P, 0, 0,
            dm.data_ptr(), dn.data_ptr())
    else:
        t = _pack(sides, cap)
        side = dict(desc=t["desc"].data_ptr(), kps=t["kps"].data_ptr(), counts=t["cnt"].data_ptr(),
                    fv_nodes=t["nodes"].data_ptr(), fv_off=t["off"].data_ptr(),
                    fv_feats=t["feats"].data_ptr(), nfv=t["nfv"].data_ptr())
        K = L.BowFrames(valid=t["flag"].data_ptr(), **side)
        F = L.BowFrames(valid=t["flag"].data_ptr() if kind == "bowkf" else None, **side)
        fn = (lib.orbg_search_by_bow_kf_batch_device if kind == "bowkf"
              else lib.orbg_search_by_bow_batch_device)
        _sync()
        rc = fn(ctx.handle, C.byref(K), C.byref(F), cap, C.c_void_p(i1.data_ptr()),
                C.c_void_p(i2.data_ptr()), P, 0.75, 0, C.c_void_p(dm.data_ptr()),
                C.c_void_p(dn.data_ptr()))
    assert rc == expect_rc, (rc, L.last_error())
    ctx.sync()
    return dm.cpu().numpy().reshape(P, cap), dn.cpu().numpy()


def _fv_scenes(kind):
    """Pairs of different counts, nnratio 0.75 and no rotation filter, plus an empty KeyFrame
    on either side."""
    names = ["chunks", "shared", "walk", "second", "invalid", "join1025"]
    sc = [S.scene("%s_%s" % (kind, n)) for n in names]
    if kind == "tri":
        sc += [S.scene("tri_geometry"), S.scene("tri_degenerate_line")]
    base = sc[1]
    sc.append(dict(base, s1=EMPTY_SIDE))
    sc.append(dict(base, s2=EMPTY_SIDE))
    return sc


def _check_fv(kind, scenes, got, gn, cap):
    for p, s in enumerate(scenes):
        n, ref = S.outputs(S.run_ref(s), kind)
        rows = len(ref)
        assert gn[p] == n, p
        assert np.array_equal(got[p, :rows], ref), p
        assert np.all(got[p, rows:] == -9), p           # rows past the count: untouched
    assert sum(int(x) for x in gn) > 0


@pytest.mark.parametrize("kind", S.FV_KINDS)
def test_fv_batch_device(kind):
    scenes = _fv_scenes(kind)
    cap = 2600
    got, gn = fv_batch(kind, scenes, cap)
    _check_fv(kind, scenes, got, gn, cap)
    counts = {len(s["s1"]["kps"]) for s in scenes}
    assert 0 in counts and len(counts) >= 5


@pytest.mark.parametrize("kind", ("bow", "bowkf"))
def test_bow_capacity(kind):
    """cap = 4096 is the last the taken mask covers; 4097 is refused before any launch."""
    from orb_slam2_test_amd import _lib as L
    scenes = [S.scene("%s_%s" % (kind, n)) for n in ("chunks", "shared")]
    got, gn = fv_batch(kind, scenes, 4096)
    _check_fv(kind, scenes, got, gn, 4096)
    got, gn = fv_batch(kind, scenes, 4097, expect_rc=L.ORBG_ENOTSUP)
    assert np.all(got == -9) and np.all(gn == -9)


# ---------------------------------------------------------------- the grid entries
def fuse_batch(scenes, cap, sim3, expect_rc=0, mcap=None):
    from orb_slam2_test_amd import _lib as L
    P = len(scenes)
    mcap = max([len(s["mps"]) for s in scenes] + [1]) + 7 if mcap is None else mcap
    t = _pack([s["kf"] for s in scenes], cap)
    cams = np.zeros(P, L.FRUSTUM_DTYPE)
    mps = np.zeros((P, mcap), L.MAPPOINT_DTYPE)
    md = np.zeros((P, mcap, 32), np.uint8)
    mc = np.zeros(P, np.int32)
    for p, s in enumerate(scenes):
        k = len(s["mps"])
        mps[p, :k], md[p, :k], mc[p], cams[p] = s["mps"], s["mdesc"], k, s["fcam"]
    d = {k: _dev(v) for k, v in dict(cams=cams, mps=mps, md=md, mc=mc).items()}
    K = L.KeyFrames(t["desc"].data_ptr(), t["kps"].data_ptr(),
                    None if sim3 else t["ur"].data_ptr(), None, t["cnt"].data_ptr(), None, None,
                    None, None)
    kfi = _dev(np.arange(P, dtype=np.int32))
    bi, bd, nf = _fill(P * mcap), _fill(P * mcap), _fill(P)
    ctx = _ctx()
    fn = L.lib().orbg_fuse_sim3_batch_device if sim3 else L.lib().orbg_fuse_batch_device
    _sync()
    rc = fn(ctx.handle, C.byref(K), cap, kfi.data_ptr(), d["cams"].data_ptr(),
            d["mps"].data_ptr(), d["md"].data_ptr(), d["mc"].data_ptr(), mcap, P, 4.0,
            bi.data_ptr(), bd.data_ptr(), nf.data_ptr())
    assert rc == expect_rc, (rc, L.last_error())
    ctx.sync()
    return (bi.cpu().numpy().reshape(P, mcap), bd.cpu().numpy().reshape(P, mcap),
            nf.cpu().numpy())


def _check_fuse(scenes, got):
    bi, bd, nf = got
    for p, s in enumerate(scenes):
        n, rbi, rbd = S.outputs(S.run_ref(s), s["kind"])
        k = len(rbi)
        assert nf[p] == n, p
        assert np.array_equal(bi[p, :k], rbi) and np.array_equal(bd[p, :k], rbd), p
        assert np.all(bi[p, k:] == -9) and np.all(bd[p, k:] == -9), p
    assert sum(int(x) for x in nf) > 0


def _fuse_scenes(kind):
    """th = 4 scenes of different keypoint and point counts, an empty KeyFrame and an empty
    point list."""
    sc = [S.scene("%s_designed_%s" % (kind, b)) for b in ("img", "tum1", "pow2")]
    sc.append(dict(sc[0], kf=dict(kps=sc[0]["kf"]["kps"][:0], desc=sc[0]["kf"]["desc"][:0],
                                  uright=None if sc[0]["kf"]["uright"] is None
                                  else sc[0]["kf"]["uright"][:0])))
    sc.append(dict(sc[1], mps=sc[1]["mps"][:0], mdesc=sc[1]["mdesc"][:0]))
    return sc


@pytest.mark.parametrize("kind", ("fuse", "fuse_sim3"))
def test_fuse_batch_device(kind):
    scenes = _fuse_scenes(kind)
    _check_fuse(scenes, fuse_batch(scenes, 300, kind == "fuse_sim3"))


def sim3_batch(scenes, cap, expect_rc=0):
    from orb_slam2_test_amd import _lib as L
    P = len(scenes)
    sides = [dict(s[k], ok=None) for s in scenes for k in ("kf1", "kf2")]
    t = _pack(sides, cap)
    mps = np.zeros((2 * P, cap), L.MAPPOINT_DTYPE)
    md = np.zeros((2 * P, cap, 32), np.uint8)
    am1 = np.zeros((P, cap), np.uint8)
    am2 = np.zeros((P, cap), np.uint8)
    for p, s in enumerate(scenes):
        n1, n2 = len(s["mp1"]), len(s["mp2"])
        mps[2 * p, :n1], md[2 * p, :n1] = s["mp1"], s["md1"]
        mps[2 * p + 1, :n2], md[2 * p + 1, :n2] = s["mp2"], s["md2"]
        am1[p, :n1], am2[p, :n2] = s["matched1"], s["matched2"]
    pairs = np.zeros(P, L.SIM3_PAIR_DTYPE)
    for p, s in enumerate(scenes):
        pairs[p] = s["g"]
    d = {k: _dev(v) for k, v in dict(mps=mps, md=md, am1=am1, am2=am2, pairs=pairs).items()}
    K = L.KeyFrames(t["desc"].data_ptr(), t["kps"].data_ptr(), None, None, t["cnt"].data_ptr(),
                    None, None, None, None)
    i1 = _dev(np.arange(0, 2 * P, 2, dtype=np.int32))
    i2 = _dev(np.arange(1, 2 * P, 2, dtype=np.int32))
    out, nf = _fill(P * cap), _fill(P)
    ctx = _ctx()
    _sync()
    rc = L.lib().orbg_search_by_sim3_batch_device(
        ctx.handle, C.byref(K), cap, i1.data_ptr(), i2.data_ptr(), d["pairs"].data_ptr(),
        d["mps"].data_ptr(), d["md"].data_ptr(), d["am1"].data_ptr(), d["am2"].data_ptr(), P, 4.0,
        out.data_ptr(), nf.data_ptr())
    assert rc == expect_rc, (rc, L.last_error())
    ctx.sync()
    return out.cpu().numpy().reshape(P, cap), nf.cpu().numpy()


def _check_sim3(scenes, got):
    out, nf = got
    for p, s in enumerate(scenes):
        n, ref = S.outputs(S.run_ref(s), "sim3")
        k = len(ref)
        assert nf[p] == n and np.array_equal(out[p, :k], ref), p
        assert np.all(out[p, k:] == -9), p
    assert sum(int(x) for x in nf) > 0


def _empty_kf2(s):
    return dict(s, kf2=dict(kps=s["kf2"]["kps"][:0], desc=s["kf2"]["desc"][:0]), mp2=s["mp2"][:0],
                md2=s["md2"][:0], matched2=s["matched2"][:0])


def test_sim3_batch_device():
    scenes = [S.scene("sim3_designed_" + b) for b in ("img", "tum1", "pow2")]
    scenes.append(_empty_kf2(scenes[0]))
    _check_sim3(scenes, sim3_batch(scenes, 300))


# ---------------------------------------------------------------- capacity
@pytest.mark.parametrize("cap", [4436, 4437, 8192])
@pytest.mark.parametrize("kind", ("fuse", "fuse_sim3", "sim3"))
def test_grid_capacity(kind, cap):
    """4436 is the last capacity whose grid fits 64 KiB of LDS; 4437 and 8192 take the opt-in
    path.  One small designed scene at the front of the slots."""
    s = S.scene(kind + "_designed_img")
    assert len(s["kf2" if kind == "sim3" else "kf"]["kps"]) <= 300
    if kind == "sim3":
        _check_sim3([s], sim3_batch([s], cap))
    else:
        _check_fuse([s], fuse_batch([s], cap, kind == "fuse_sim3"))


@pytest.mark.parametrize("kind", ("fuse", "fuse_sim3", "sim3"))
def test_grid_capacity_refused(kind):
    from orb_slam2_test_amd import _lib as L
    s = S.scene(kind + "_designed_pow2")
    if kind == "sim3":
        out, nf = sim3_batch([s], 8193, expect_rc=L.ORBG_ENOTSUP)
        assert np.all(out == -9) and np.all(nf == -9)
    else:
        bi, bd, nf = fuse_batch([s], 8193, kind == "fuse_sim3", expect_rc=L.ORBG_ENOTSUP)
        assert np.all(bi == -9) and np.all(bd == -9) and np.all(nf == -9)
