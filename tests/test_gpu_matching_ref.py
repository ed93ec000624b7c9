"""GPU: the tracking matchers and stereo matching (HIP, through the C ABI) against
tests/ref_matching.py, not the oracle.

The scenes of matching_scenes.py (synthetic keypoints up to the image border, non-integer
bounds, forced ties, taken keypoints, designed uRight and rotation cases, counts around the
kernels' chunk sizes) go through ORBmatcher.SearchForInitialization and both
ORBmatcher.SearchByProjection overloads and must equal the reference exactly; one call of
orbg_search_by_projection_batch_device takes three frames of different counts and bounds,
one of them empty.  Stereo runs extract_batch_device + stereo_batch_device at 320x240 and the
reference is fed the downloaded keypoints, descriptors and pyramid levels.
"""
import ctypes as C

import numpy as np
import pytest

import matching_scenes as MS
from test_matching_ref import BF, FX, H, NFEAT, STEREO_SEEDS, W, check_stereo, stereo_ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", MS.SCENE_NAMES)
def test_kernels_equal_reference(name):
    s = MS.scene(name)
    MS.check_equal(MS.run_gpu(s), s, name)


def test_batch_device_three_frames():
    import torch
    from orb_slam2_test_amd import _lib as L
    from orb_slam2_test_amd.orbmatcher import _ctx
    scenes = [MS.scene(n) for n in ("last_img", "last_0_5", "last_dist")]
    assert all(s["th"] == 15.0 and s["ori"] and s["taken"] is None for s in scenes)
    B = len(scenes)
    fc = max(len(s["kps"]) for s in scenes)
    qc = max(len(s["pts"]) for s in scenes)
    kps = np.zeros((B, fc), L.KP_DTYPE)
    desc = np.zeros((B, fc, 32), np.uint8)
    ur = np.full((B, fc), -1.0, np.float32)
    q = np.zeros((B, qc), L.LF_DTYPE)
    qd = np.zeros((B, qc, 32), np.uint8)
    cnt, qcnt = np.zeros(B, np.int32), np.zeros(B, np.int32)
    bounds = np.zeros((B, 4), np.float32)
    cams = (L.TrackCamera * B)()
    for f, s in enumerate(scenes):
        n, m = len(s["kps"]), len(s["pts"])
        kps[f, :n], desc[f, :n] = s["kps"], s["desc"]
        if s["uright"] is not None:
            ur[f, :n] = s["uright"]
        q[f, :m], qd[f, :m] = s["pts"], s["pdesc"]
        cnt[f], qcnt[f], bounds[f] = n, m, s["bounds"]
        c = s["cam"]
        cams[f] = L.track_camera(c["Tcw"], c["Tlw"], c["fx"], c["fy"], c["cx"], c["cy"], c["bf"],
                                 c["b"], c["mono"])
    dev = "cuda"
    t = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).to(dev)
         for k, v in dict(kps=kps, desc=desc, ur=ur, q=q, qd=qd, cnt=cnt, qcnt=qcnt,
                          bounds=bounds).items()}
    cam_t = torch.from_numpy(np.frombuffer(bytes(cams), np.uint8).copy()).to(dev)
    match = torch.full((B * fc,), -7, dtype=torch.int32, device=dev)
    nm = torch.zeros(B, dtype=torch.int32, device=dev)
    tb = L.TrackBatch()
    tb.kps, tb.desc, tb.uright = t["kps"].data_ptr(), t["desc"].data_ptr(), t["ur"].data_ptr()
    tb.taken0 = None
    tb.counts, tb.bounds, tb.frame_cap = t["cnt"].data_ptr(), t["bounds"].data_ptr(), fc
    tb.queries, tb.qdesc = t["q"].data_ptr(), t["qd"].data_ptr()
    tb.qcounts, tb.query_cap = t["qcnt"].data_ptr(), qc
    tb.cams, tb.th, tb.nnratio, tb.check_ori = cam_t.data_ptr(), 15.0, 0.0, 1
    tb.match, tb.nmatches = match.data_ptr(), nm.data_ptr()
    ctx = _ctx(0)
    torch.cuda.synchronize()
    L.check(L.lib().orbg_search_by_projection_batch_device(ctx.handle, L.TRACK_LASTFRAME,
                                                           C.byref(tb), B), "batch")
    ctx.sync()
    match = match.cpu().numpy().reshape(B, fc)
    nm = nm.cpu().numpy()
    for f, s in enumerate(scenes):
        MS.check_equal((int(nm[f]), match[f, :cnt[f]], None), s, "frame %d" % f)


# ---------------------------------------------------------------- stereo
@pytest.fixture(scope="module")
def stereo_images():
    from orb_slam2_test_amd import synthetic as S
    pairs = [S.stereo_pair(H, W, seed=seed, d_max=30.0)[:2] for seed in STEREO_SEEDS]
    L0 = pairs[0][0]
    return pairs + [(L0, L0.copy()), (L0, S.constant(H, W, 90))]


def run_stereo(pairs, min_z=BF / FX):
    """Each pair through extract_batch_device + stereo_batch_device; the reference on the
    downloaded keypoints, descriptors and pyramid levels.  Returns [(ur, dp, ref)]."""
    import torch
    from orb_slam2_test_amd import ORBextractor
    frames = np.stack([im for pr in pairs for im in pr])
    ext = ORBextractor(NFEAT, 1.2, 8, 20, 7, max_batch=len(frames))
    d = torch.from_numpy(frames).cuda()
    ext.extract_batch_device(d.data_ptr(), len(frames), W, H)
    n = len(pairs)
    ext.stereo_batch_device(np.arange(n) * 2, np.arange(n) * 2 + 1, BF, min_z)
    out = []
    for i in range(n):
        side = []
        for f in (2 * i, 2 * i + 1):
            k, dsc = ext.download_frame(f)
            side.append(dict(kps=k, desc=dsc, pyramid=[ext.get_level(f, l) for l in range(8)]))
        ur, dp, nv = ext.download_stereo(i, len(side[0]["kps"]))
        assert nv == int((dp > 0).sum())
        out.append((ur, dp, stereo_ref(side[0], side[1], min_z=min_z)))
    ext.close()
    return out


def test_stereo_kernels_within_bounds_of_reference(stereo_images):
    res = run_stereo(stereo_images)
    for ur, dp, r in res[:2]:
        eu, ed, n = check_stereo(ur, dp, r, cap=0.01)
        print("flagged %d of %d, matched %d, max |duR| %.3g, max rel depth %.3g"
              % (len(r.flagged), len(ur), n, eu, ed))
        assert n > 100
    ur, dp, r = res[2]      # identical images: median 0 clears every match
    assert len(r.pre) > 100 and np.all(r.depth == -1) and np.all(dp == -1) and np.all(ur == -1)
    ur, dp, r = res[3]      # featureless right image
    assert not r.pre and np.all(dp == -1) and np.all(ur == -1)


def test_stereo_no_disparity_limit(stereo_images):
    for ur, dp, r in run_stereo(stereo_images[:1], min_z=0.0):
        check_stereo(ur, dp, r, cap=0.01)


@pytest.mark.parametrize("env", [{"ORBG_ST_FUSED": "0"}, {"ORBG_ST_LCAP": "64"}])
def test_stereo_match_paths(stereo_images, monkeypatch, env):
    """The two-kernel path and the fused kernel's global-list path (both knobs are read at
    launch time)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for ur, dp, r in run_stereo(stereo_images[:2]):
        _, _, n = check_stereo(ur, dp, r, cap=0.01)
        assert n > 100
