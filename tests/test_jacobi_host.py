"""CPU: the bits of the solvers that sit on csrc/jacobi.h.  lib/jacobi_host (csrc/jacobi_host.hip)
calls sim3_horn, pnp_control_points, pnp_polar3, the EPnP chain through pnp_tail,
init_hypothesis, init_svd3 and init_triangulate on seeded and degenerate inputs and prints every
output value exactly, one section per entry point.  The functions are __host__ __device__ and
the build forbids contraction, so these are the kernels' statements; only sqrt, fabs and IEEE
arithmetic are involved, so the output is the same on every x86-64 host.

DIGESTS holds the SHA-256 of each section as printed by the same program built against the
headers of commit 0e862c0, the last one where Sim3Solver, PnPsolver and Initializer each carried
their own Jacobi solves.  A change to the shared solves that moves one bit of any of them fails
here.
"""
import hashlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JACOBI_HOST = os.path.join(ROOT, "orb_slam2_test_amd", "lib", "jacobi_host")

DIGESTS = {
    "sim3_horn": "ed72f73854543eb459b2ea2b14997c66e18eb99212af7988c50941e45c184143",
    "pnp_control_points": "e74468f4a9d43a3e692b066bb69f356d11bcedc6569a18103e9cc480e094abb0",
    "pnp_polar3": "8c60f95b97caef5143f38508021e1029463ef92352f00ed6cd5f624e41bfd1d8",
    "pnp_tail": "f2e1b32eade10269402c7c0dd0b8a160e487f2021674f95529cc378ef5a0125b",
    "init_hypothesis": "8a92bfe8e1b40a21a3b27a8a46bde4ba1814d7557ca5bb2776759d220a97cb91",
    "init_svd3": "cfe110e94c0291d712c719580fe816ae7402ce8c175d2595970ce70c387465e3",
    "init_triangulate": "18d976272d6e10a0ae1c7f2fef92a009192250ced459f4d5afb91c718b4bc674",
}


@pytest.fixture(scope="module")
def sections():
    """section name -> its lines, from one run of the program"""
    out, name = {}, None
    for line in subprocess.check_output([JACOBI_HOST], text=True).splitlines():
        if line.startswith("["):
            name = line.strip("[]")
            out[name] = []
        else:
            out[name].append(line)
    return out


def test_sections_are_the_pinned_ones(sections):
    assert list(sections) == list(DIGESTS)
    assert all(len(v) >= 40 for v in sections.values())


@pytest.mark.parametrize("name", list(DIGESTS))
def test_section_bits(sections, name):
    assert hashlib.sha256("\n".join(sections[name]).encode()).hexdigest() == DIGESTS[name]
