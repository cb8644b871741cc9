"""The fast tier's control step in substep chunks, on the CPU: the planner's arithmetic (uhc_amd/csrc/uhc_plan.cpp: plan_fast_chunks, fast_chunk_range,
default_fast_chunk, the UHC_FAST_CHUNK knob) compiled with the host compiler beside tests/fast_chunks_probe.cpp.

The kernel (uhc_step_kernel<0, 1, *>) computes chunk c's substeps as [c chunk, min((c + 1) chunk, n_substeps)) and the host launches n_chunks x n_env
workgroups, all of which the general tier's consumers wait for: the chunks must cover the step exactly once and in order, and the sizes must be
n_chunks x n_env; a chunk size of 0 or of the whole step must give the whole-step launch's sizes."""
import ctypes as C
import os

import pytest

from tests import probe_build

N_SUBSTEPS = 15
CHUNKS = (0, 1, 3, 5, 7, 8, 15, 16)
N_ENVS = (1, 64, 1024, 4096)
KIB = 1024


def build_probe():
    return probe_build.build_probe("fast_chunks_probe.so", ["tests/fast_chunks_probe.cpp", "uhc_amd/csrc/uhc_plan.cpp"],
                                   ["uhc_amd/csrc/" + h for h in ("uhc_plan.h", "uhc_host.h", "uhc_device.h", "uhc_step_words.h")] + ["include/uhc_amd.h"], probe_build.HIP_STRUCT_FLAGS)


@pytest.fixture(scope="module")
def L():
    lib = C.CDLL(build_probe())
    lib.uhc_fc_knob.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    return lib


def plan(L, n_substeps, chunk, n_env):
    o = (C.c_int * 4)()
    L.uhc_fc_plan(n_substeps, chunk, n_env, o)
    return dict(zip(("chunk", "n_chunks", "grid", "prod_total"), o))


def ranges(L, n_substeps, chunk, n_env, n_chunks):
    out = []
    for c in range(n_chunks):
        r = (C.c_int * 2)()
        L.uhc_fc_range(n_substeps, chunk, n_env, c, r)
        out.append((r[0], r[1]))
    return out


@pytest.mark.parametrize("chunk", CHUNKS)
def test_chunks_cover_the_step_once_and_in_order(L, chunk):
    for n_env in N_ENVS:
        p = plan(L, N_SUBSTEPS, chunk, n_env)
        rs = ranges(L, N_SUBSTEPS, chunk, n_env, p["n_chunks"])
        assert rs[0][0] == 0 and rs[-1][1] == N_SUBSTEPS
        for (a0, a1), (b0, b1) in zip(rs, rs[1:]):
            assert a1 == b0
        assert all(lo < hi for lo, hi in rs)  # no empty chunk: no workgroup that only waits
        assert [s for lo, hi in rs for s in range(lo, hi)] == list(range(N_SUBSTEPS))
        # what the kernel computes from KernelArgs::chunk alone
        if p["chunk"]:
            assert rs == [(c * p["chunk"], min((c + 1) * p["chunk"], N_SUBSTEPS)) for c in range(p["n_chunks"])]
            assert all(hi - lo <= p["chunk"] for lo, hi in rs)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_grid_and_prod_total(L, chunk):
    for n_env in N_ENVS:
        p = plan(L, N_SUBSTEPS, chunk, n_env)
        assert p["grid"] == p["prod_total"] == p["n_chunks"] * n_env
        want = 1 if chunk in (0, 15, 16) else -(-N_SUBSTEPS // chunk)
        assert p["n_chunks"] == want


@pytest.mark.parametrize("chunk", (0, 15, 16, -3))
def test_one_chunk_is_the_whole_step_launch(L, chunk):
    for n_env in N_ENVS:
        assert plan(L, N_SUBSTEPS, chunk, n_env) == dict(chunk=0, n_chunks=1, grid=n_env, prod_total=n_env)


def knob(L, value):
    o = (C.c_int * 2)()
    L.uhc_fc_knob(None if value is None else value.encode(), o)
    return o[0], bool(o[1])


def test_knob(L):
    assert knob(L, None) == (0, False)
    for v in (1, 3, 5, 8, 15, 16):
        assert knob(L, str(v)) == (v, False)
    got, bad = knob(L, "0")  # "0": one chunk, said explicitly (not "unset")
    assert not bad and got >= N_SUBSTEPS
    for v in ("-1", "-5", "abc", "", "3x", "2.5", " "):
        assert knob(L, v)[1], v


def test_a_bad_knob_refuses_the_batch():
    from tests.test_batch_plan_cpu import Probe, build_probe as build_plan_probe, model_class
    model, ctrl = model_class("asset")
    P = Probe(build_plan_probe())
    for v in ("-1", "abc"):
        os.environ["UHC_FAST_CHUNK"] = v
        try:
            with pytest.raises(RuntimeError, match="UHC_FAST_CHUNK"):
                P.plan(model, ctrl, 64)
        finally:
            del os.environ["UHC_FAST_CHUNK"]
    os.environ["UHC_FAST_CHUNK"] = "5"
    try:
        P.plan(model, ctrl, 64)
    finally:
        del os.environ["UHC_FAST_CHUNK"]


def test_default_follows_the_places(L):
    # 256 CUs: 768 places of the 52 KiB layout, 1024 of the 40 KiB one.  A batch that fits at once keeps the whole-step launch.
    d = L.uhc_fc_default
    assert d(0, 15, 1024, 256, 52 * KIB) > 0
    assert d(0, 15, 768, 256, 52 * KIB) == 0
    assert d(0, 15, 1024, 256, 40 * KIB) == 0
    assert d(0, 15, 4096, 256, 40 * KIB) > 0
    assert d(0, 15, 64, 256, 52 * KIB) == 0
    for k in (1, 3, 5, 8):  # the knob wins, whatever the batch
        assert d(k, 15, 64, 256, 52 * KIB) == k and d(k, 15, 4096, 256, 40 * KIB) == k
    assert d(15, 15, 4096, 256, 40 * KIB) == 0 and d(0x7fff, 15, 4096, 256, 40 * KIB) == 0
    assert d(0, 1, 4096, 256, 40 * KIB) == 0  # a one-substep control step has nothing to split


def test_sticky_step_carries_the_chunk_plan(L):
    o = (C.c_int * 4)()
    L.uhc_fc_sticky(1024, 256, 52 * KIB, 3, 15, o)
    assert list(o) == [3, 5, 5 * 1024, 5 * 1024]
    L.uhc_fc_sticky(1024, 256, 52 * KIB, 0, 0, o)  # fields at zero: as before
    assert list(o) == [0, 1, 1024, 1024]
    L.uhc_fc_sticky(1024, 256, 52 * KIB, 15, 15, o)
    assert list(o) == [0, 1, 1024, 1024]
