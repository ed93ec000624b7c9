"""GPU: the device Optimizer::OptimizeEssentialGraph (csrc/essential_kernels.hip behind
orbg_optimize_essential_graph, the orbg_eg_graph entry points and orbg_eg_correct_points_device,
and the Python functions on top) against the float64 reference of tests/ref_essential.py: every
vertex within EG_TOL of the reference's, the final chi2 no more than EG_TOL (relative) above
it.  What is exact is checked exactly: the fixed vertex and, under fix scale, every scale are
the input's bits; Tiw is the returned estimate rounded once; two runs and the two entry points
agree bit for bit; an error return leaves the outputs alone.

tests/test_essential_ref.py holds the CPU side of the premises (EG_TOL is measured there).
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_essential as E  # noqa: E402
from test_essential_ref import vertex_distance  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = list(E.CASES)
RUN = [k for k in NAMES if k not in ("n1", "e0")]


@pytest.fixture(scope="module")
def O():
    from orb_slam2_test_amd import optimizer
    return optimizer


@pytest.fixture(scope="module")
def L():
    from orb_slam2_test_amd import _lib
    return _lib


def records(L, S):
    out = np.zeros(len(S[2]), L.SIM3D_DTYPE)
    out["q"], out["t"], out["s"] = S
    return out


def edges_of(L, sc):
    e = np.zeros(len(sc["edges"]), L.EG_EDGE_DTYPE)
    e["i"], e["j"], e["kind"] = sc["edges"][:, 0], sc["edges"][:, 1], sc["edges"][:, 2]
    return e


@pytest.fixture(scope="module")
def host(O, L):
    """name -> (Siw, Tiw, report) of the host entry, run once."""
    out = {}
    for k in NAMES:
        sc = E.case(k)[0]
        out[k] = O.OptimizeEssentialGraph(records(L, sc["Scw"]), records(L, sc["Snc"]), edges_of(L, sc),
                                          sc["fixed"], sc["fix_scale"])
    return out


@pytest.mark.parametrize("name", RUN)
def test_case_against_the_reference(L, host, name):
    sc, ref = E.case(name)
    Siw, Tiw, rep = host[name]
    got = dict(q=Siw["q"], t=Siw["t"], s=Siw["s"])
    d = vertex_distance(got, ref)
    chi = E.final_chi2(sc, (got["q"], got["t"], got["s"]))
    print(name, "distance %.3g" % d, "chi2 %.9g (reference %.9g, excess %.3g)"
          % (chi, ref["chi2"][1], chi / ref["chi2"][1] - 1), "iterations", rep["iterations"], "trials",
          rep["trials"], "terminated", rep["terminated"], "reference", ref["iterations"], ref["trials"],
          ref["stop"])
    assert d <= E.EG_TOL
    assert chi <= ref["chi2"][1] * (1 + E.EG_TOL)
    assert abs(rep["final_chi2"] - chi) <= 1e-9 * chi and rep["initial_chi2"] > rep["final_chi2"]
    assert 1 <= rep["iterations"] <= E.ITERATIONS
    f = sc["fixed"]
    inp = records(L, sc["Scw"])
    assert Siw[f].tobytes() == inp[f].tobytes()              # the fixed vertex: the input's bits
    if sc["fix_scale"]:
        assert Siw["s"].tobytes() == inp["s"].tobytes()      # every scale: the input's bits
    else:
        assert not np.array_equal(np.delete(Siw["s"], f), np.delete(inp["s"], f))


@pytest.mark.parametrize("name", NAMES)
def test_tiw_is_the_estimate_rounded_once(host, name):
    Siw, Tiw, _ = host[name]
    want = E.poses((Siw["q"], Siw["t"], Siw["s"]))
    assert Tiw.dtype == np.float32 and Tiw.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", ["n1", "e0"])
def test_nothing_to_optimise_returns_the_input(L, host, name):
    sc = E.case(name)[0]
    Siw, _, rep = host[name]
    assert rep["iterations"] == 0 and rep["trials"] == 0
    assert Siw.tobytes() == records(L, sc["Scw"]).tobytes()


def test_two_calls_and_the_two_entry_points_agree_bit_for_bit(O, L, host):
    for name in ("ring24_mid", "ring256", "ring12_fs"):
        sc = E.case(name)[0]
        a = O.OptimizeEssentialGraph(records(L, sc["Scw"]), records(L, sc["Snc"]), edges_of(L, sc),
                                     sc["fixed"], sc["fix_scale"])
        g = O.EssentialGraph(edges_of(L, sc), sc["n"], sc["fixed"])
        b = g.optimize(records(L, sc["Scw"]), records(L, sc["Snc"]), sc["fix_scale"])
        b2 = g.optimize(records(L, sc["Scw"]), records(L, sc["Snc"]), sc["fix_scale"])
        g.close()
        for r in (a, b, b2):
            assert r[0].tobytes() == host[name][0].tobytes(), name
            assert r[1].tobytes() == host[name][1].tobytes(), name
            assert r[2] == host[name][2], name


def test_graph_info_counts_blocks(O, L):
    for name in ("ring12", "ring24_mid", "ring256"):
        sc = E.case(name)[0]
        g = O.EssentialGraph(edges_of(L, sc), sc["n"], sc["fixed"])
        nfree, hb, lb = g.info()
        g.close()
        f = sc["fixed"]
        pairs = {tuple(sorted(p)) for p in sc["edges"][:, :2].tolist() if f not in p}
        print(name, nfree, hb, lb)
        assert nfree == sc["n"] - 1 and hb == nfree + len(pairs) and hb <= lb <= L.EG_MAX_BLOCKS
    assert lb > hb     # ring256: the loop's edges fill in


def test_correct_map_points(O, L, host):
    import torch
    from orb_slam2_test_amd.orbmatcher import _ctx
    sc = E.case("ring40")[0]
    Siw = host["ring40"][0]
    rng = np.random.default_rng(21)
    n = 1000
    ref = rng.integers(0, sc["n"], n).astype(np.int32)
    pts = (rng.normal(size=(n, 3)) * 8).astype(np.float32)
    want = E.correct_points(sc["Scw"], (Siw["q"], Siw["t"], Siw["s"]), ref, pts)
    got = O.CorrectMapPoints(records(L, sc["Scw"]), Siw, ref, pts)
    assert got.dtype == np.float32 and got.shape == (n, 3)
    w32 = want.astype(np.float32)
    # the double arithmetic differs by about 1e-15: only the rounding boundary can differ
    assert (np.abs(got.astype(np.float64) - w32) <= np.spacing(np.abs(w32))).all()
    assert (got == w32).mean() > 0.99
    moved = np.abs(got - pts).max()
    assert moved > 1e-3

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d_c, d_s, d_r, d_p = up(records(L, sc["Scw"])), up(Siw), up(ref), up(pts)
    d_o = torch.full((n * 12 + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx = _ctx(0)
    m = n - 37
    L.check(L.lib().orbg_eg_correct_points_device(ctx.handle, d_c.data_ptr(), d_s.data_ptr(), sc["n"],
                                                  d_r.data_ptr(), d_p.data_ptr(), m, d_o.data_ptr()),
            "orbg_eg_correct_points_device")
    ctx.sync()
    raw = d_o.cpu().numpy()
    assert (raw[m * 12:] == 0xAB).all()                      # bytes past n are untouched
    assert raw[:m * 12].tobytes() == got[:m].tobytes()


def test_errors_leave_the_outputs_untouched(L):
    from orb_slam2_test_amd.orbmatcher import _ctx
    h = _ctx(0).handle
    sc = E.case("ring12")[0]
    Scw, Snc, e = records(L, sc["Scw"]), records(L, sc["Snc"]), edges_of(L, sc)
    n = sc["n"]

    def call(Scw, Snc, e, nedge, nvert, fixed):
        Siw = np.zeros(max(nvert, 1), L.SIM3D_DTYPE)
        Siw.view(np.uint8)[:] = 0xCD
        Tiw = np.full((max(nvert, 1), 12), np.float32(7.5))
        rep = L.LmReport()
        rep.iterations = -3
        rc = L.lib().orbg_optimize_essential_graph(h, L.ptr(Scw), L.ptr(Snc), nvert, L.ptr(e), nedge,
                                                   fixed, 0, 20, L.ptr(Siw), L.ptr(Tiw),
                                                   ctypes.byref(rep))
        assert (Siw.view(np.uint8) == 0xCD).all() and (Tiw == 7.5).all() and rep.iterations == -3
        return rc
    assert call(None, Snc, e, len(e), n, 0) == L.ORBG_EINVAL
    assert call(Scw, None, e, len(e), n, 0) == L.ORBG_EINVAL
    assert call(Scw, Snc, None, len(e), n, 0) == L.ORBG_EINVAL
    for fixed in (-1, n):
        assert call(Scw, Snc, e, len(e), n, fixed) == L.ORBG_EINVAL
    for field, value in (("i", n), ("j", -1), ("kind", 2), ("kind", -1)):
        e2 = e.copy()
        e2[field][5] = value
        assert call(Scw, Snc, e2, len(e), n, 0) == L.ORBG_EINVAL
    e2 = e.copy()
    e2["j"][7] = e2["i"][7]
    assert call(Scw, Snc, e2, len(e), n, 0) == L.ORBG_EINVAL
    assert L.lib().orbg_optimize_essential_graph(h, L.ptr(Scw), L.ptr(Snc), n, L.ptr(e), len(e), 0, 0,
                                                 20, None, None, None) == L.ORBG_EINVAL
    # more blocks of H than a graph may have: a clique of 726 vertices (725 free)
    nv = 726
    iu = np.triu_indices(nv, 1)
    big = np.zeros(len(iu[0]), L.EG_EDGE_DTYPE)
    big["i"], big["j"], big["kind"] = iu[1], iu[0], 1
    assert len(big) - (nv - 1) + (nv - 1) > L.EG_MAX_BLOCKS
    S = np.zeros(nv, L.SIM3D_DTYPE)
    S["q"][:, 3] = 1
    S["s"] = 1
    assert call(S, S, big, len(big), nv, 0) == L.ORBG_ENOTSUP
    g = ctypes.c_void_p()
    assert L.lib().orbg_eg_graph_create(h, L.ptr(big), len(big), nv, 0, ctypes.byref(g)) == L.ORBG_ENOTSUP
    assert not g.value
    assert L.lib().orbg_eg_graph_create(h, L.ptr(e), len(e), n, n, ctypes.byref(g)) == L.ORBG_EINVAL
    assert L.lib().orbg_eg_correct_points_device(h, None, None, n, None, None, 5, None) == L.ORBG_EINVAL


def test_public_exports():
    import orb_slam2_test_amd as pkg
    for name in ("OptimizeEssentialGraph", "CorrectMapPoints", "EssentialGraph"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
