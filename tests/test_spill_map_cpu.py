"""tools/spill_map.py's parser on a small assembly text (tests/golden/spill_map_snippet.s, written for this test in the compiler's format): spill stores and
reloads by kernel, by stage of the inline chain, inside / outside a loop closed by a long branch, and the spill figures of the code-object metadata.
No compiler runs here: a step-kernel unit takes two minutes to compile."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import spill_map  # noqa: E402

SNIPPET = os.path.join(ROOT, "tests", "golden", "spill_map_snippet.s")

# the source the snippet's line numbers refer to: only the lines that begin a function matter
STAGES_H = {10: "__device__ __forceinline__ double rcp_newton(double x) {",
            20: "template <int NC>", 21: "__device__ __forceinline__ int as_solve(const int (&Alo)[64], int nefc) {",
            30: "template <int LT>", 31: "__device__ __forceinline__ int k_pgs_fast(double* S, int nefc) {",
            40: "__device__ __forceinline__ void k_euler(double* S) {",
            45: "__device__ __forceinline__ void declared_only(double* S);",
            50: "template <int MODE>", 51: "__global__ void __launch_bounds__(64) kernel(double* p) {",
            70: "__global__ void other() {}"}


def _source(path):
    if os.path.basename(path) != "stages.h":
        return None  # (a header that is not the repository's)
    return "\n".join(STAGES_H.get(n, "    x;") for n in range(1, 80))


def _parsed():
    return spill_map.parse_asm(open(SNIPPET).read())


def test_regions_of_a_source():
    regs = spill_map.regions_of(_source("stages.h"))
    assert regs == [(10, "rcp_newton"), (20, "as_solve"), (30, "k_pgs_fast"), (40, "k_euler"), (50, "kernel"), (70, "other")]
    assert spill_map.region_name(regs, 5) == "(head)"
    assert spill_map.region_name(regs, 33) == "k_pgs_fast" and spill_map.region_name(regs, 69) == "kernel"


def test_spills_per_kernel_with_frames_and_loops():
    kernels, _ = _parsed()
    assert list(kernels) == ["_Z6kernelILi1EEvPd", "_Z6otherv"]
    assert kernels["_Z6otherv"] == []
    sp = kernels["_Z6kernelILi1EEvPd"]
    assert [(s["kind"], s["bytes"], s["in_loop"]) for s in sp] == [
        ("store", 8, False), ("store", 4, False),                      # ahead of the loop
        ("reload", 4, True), ("store", 4, True), ("reload", 8, True), ("reload", 4, True),   # between the loop's label and the long branch back to it
        ("reload", 4, False)]                                           # behind it
    assert sp[0]["frames"] == [("./stages.h", 33), ("./stages.h", 52)]
    assert sp[2]["frames"] == [("./stages.h", 12), ("./stages.h", 21), ("./stages.h", 37), ("./stages.h", 56)]
    assert sp[3]["frames"][0] == ("/opt/rocm/include/hip/math.h", 784)
    assert sp[4]["frames"] == sp[3]["frames"], "a .loc with line 0 keeps the line before it"


def test_metadata_of_the_kernels():
    _, meta = _parsed()
    k = meta["_Z6kernelILi1EEvPd"]
    assert (k["private_segment_fixed_size"], k["vgpr_spill_count"], k["sgpr_spill_count"], k["vgpr_count"], k["agpr_count"]) == ("24", "4", "3", "16", "8")
    assert meta["_Z6otherv"]["private_segment_fixed_size"] == "0"
    assert "offset" not in k and "address_space" not in k, "the arguments' own keys are not the kernel's"


def test_report_attributes_to_the_stage_of_the_inline_chain():
    kernels, meta = _parsed()
    lines = spill_map.report(kernels, meta, read_source=_source, name_of=lambda s: s)
    head = [l for l in lines if l.startswith("_Z6kernel")]
    assert head == ["_Z6kernelILi1EEvPd: scratch 24 B/lane, VGPR spills 4, SGPR spills 3, vgpr 16 agpr 8 sgpr 20"]
    rows = {}
    for l in lines[:lines.index(next(l for l in lines if l.startswith("_Z6otherv")))]:
        f = l.split()
        if f and f[0] in ("stages.h", "total"):
            rows[f[1] if f[0] == "stages.h" else "total"] = [int(x) for x in f[-4:]]
    # region: stores, of them in a loop, reloads, of them in a loop
    assert rows == {"as_solve": [1, 1, 2, 2],     # rcp_newton's reload and math.h's store count for the stage they were inlined into
                    "k_euler": [0, 0, 1, 1],
                    "k_pgs_fast": [2, 0, 0, 0],
                    "kernel": [0, 0, 1, 0],
                    "total": [3, 1, 4, 3]}


def test_report_filters_by_kernel_and_bins_lines():
    kernels, meta = _parsed()
    lines = spill_map.report(kernels, meta, want="other", read_source=_source, name_of=lambda s: s)
    assert lines[0].startswith("_Z6otherv: scratch 0 B/lane") and not any("kernelILi1E" in l for l in lines)
    binned = spill_map.report(kernels, meta, want="kernelILi1E", bin_lines=10, read_source=_source, name_of=lambda s: s)
    assert any(l.split()[:3] == ["stages.h", "as_solve", "20-29"] for l in binned)
    assert any(l.split()[:3] == ["stages.h", "k_pgs_fast", "30-39"] for l in binned)
