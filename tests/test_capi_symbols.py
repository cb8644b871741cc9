"""CPU: libuhc_amd.so loads and exports every symbol include/uhc_amd.h declares (no compute calls here)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "uhc_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(uhc_[a-z_0-9A-Z]+)\s*\(", src)))


def test_header_symbols_are_exported_and_listed():
    import __graft_entry__ as g
    g.build()
    from uhc_amd import _lib
    names = _declared()
    assert len(names) >= 20 and "uhc_env_step" in names and "uhc_batch_simulate" in names
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/uhc_amd.h but not exported"
    assert set(names) == set(_lib.SYMBOLS), set(names) ^ set(_lib.SYMBOLS)
    # ... and nothing else: the launchers / accessors the translation units share (uhc_launch_*, uhc_internal_*) are not exports
    import subprocess
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted({l.split()[-1] for l in dyn.splitlines() if " T " in l and l.split()[-1].startswith("uhc_")})
    assert exported == names, sorted(set(exported) ^ set(names))
    L.uhc_abi_version.restype = ctypes.c_int32
    header = open(os.path.join(ROOT, "include", "uhc_amd.h")).read()
    assert L.uhc_abi_version() == int(re.search(r"#define UHC_ABI_VERSION (\d+)", header).group(1))
    # the shipped library is a release build: no measurement switches (UHC_DEBUG_EXP_* are compiled out and masked), no stage counters, no poison / guards
    L.uhc_build_flags.restype = ctypes.c_int32
    assert L.uhc_build_flags() == 0


def test_experiment_switches_exist_only_behind_the_build_flag():
    """The measurement switches UHC_DEBUG_EXP_* (bits 8-12: working-set fill, consumer cap, sticky tier 4) change which envs report windows / sweeps: every read of them in the kernels goes
    through UHC_EXP(name), which is `false` unless the library is built with -DUHC_EXPERIMENTS, and the host masks the bits otherwise."""
    reads = _switch_reads(os.path.join(ROOT, "uhc_amd", "csrc"))
    # what exists today, so that an empty match cannot pass: UHC_EXP x 4 at three sites of the kernels, the host's fixed_cap2, and the mask
    assert sorted(w for _, _, w in reads) == ["UHC_EXP"] * 4 + ["capi", "mask"], reads
    assert {n for _, n, w in reads if w == "UHC_EXP"} == {"UHC_DEBUG_EXP_NO_RANK_FILL", "UHC_DEBUG_EXP_FILL_48", "UHC_DEBUG_EXP_FILL_56", "UHC_DEBUG_EXP_STICKY_TIER4"}
    assert [(f, n) for f, n, w in reads if w != "UHC_EXP"] == [("uhc_capi.cpp", "UHC_DEBUG_EXP_FIXED_CAP2"), ("uhc_plan.cpp", "UHC_DEBUG_EXP_MASK")]


MASK_STATEMENT = "k.dbg &= ~UHC_DEBUG_EXP_MASK;"


def _switch_reads(csrc):
    """-> [(file, name, where)] for every occurrence of a measurement switch's name (UHC_DEBUG_EXP_*, include/uhc_amd.h) in the sources, comments stripped; asserts that
    each stands inside a UHC_EXP( ... ), in uhc_capi.cpp within 400 characters of UHC_EXPERIMENTS, or in uhc_plan.cpp's masking statement -- and that no source reads
    or sets KernelArgs::dbg by a number, which would get round the names."""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uhc_amd.h")).read(), flags=re.S)
    enum = re.search(r"enum UhcDebug \{(.*?)\};", header, flags=re.S).group(1)
    switches = re.findall(r"\b(UHC_DEBUG_EXP_\w+) = 1 << (\d+)", enum)
    assert sorted(int(b) for _, b in switches) == [8, 9, 10, 11, 12], switches  # the five measurement switches carry the prefix, and nothing else does
    assert all(not n.startswith("UHC_DEBUG_EXP_") for n, b in re.findall(r"\b(UHC_\w+) = 1 << (\d+)", enum) if int(b) < 8)
    mask = re.search(r"#define UHC_DEBUG_EXP_MASK \((.*?)\)\n", header).group(1)
    assert sorted(mask.split(" | ")) == sorted(n for n, _ in switches)  # the mask is the OR of those five names
    names = {n for n, _ in switches} | {"UHC_DEBUG_EXP_MASK"}
    out = []
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".h", ".hip", ".cpp")):
            continue
        txt = re.sub(r"/\*.*?\*/", "", re.sub(r"//.*", "", open(os.path.join(csrc, f)).read()), flags=re.S)
        m = re.search(r"dbg\s*(&|\|=|&=|\^=|>>|==)\s*~?\s*\(*\s*(0x[0-9a-fA-F]+|\d)", txt)
        assert m is None, (f, m.group(0))
        for m in re.finditer(r"\bUHC_DEBUG_EXP_\w+", txt):
            assert m.group(0) in names, (f, m.group(0))
            in_exp = re.search(r"UHC_EXP\(\s*$", txt[:m.start()]) is not None and txt[m.end():].lstrip().startswith(")")
            in_capi = f == "uhc_capi.cpp" and "UHC_EXPERIMENTS" in txt[max(0, m.start() - 400):m.end() + 400]
            a = txt.rfind(";", 0, m.start()) + 1
            in_mask = f == "uhc_plan.cpp" and txt[a:txt.find(";", m.end()) + 1].strip().endswith(MASK_STATEMENT) and "#ifndef UHC_EXPERIMENTS" in txt[max(0, a - 200):a + 200]
            assert in_exp or in_capi or in_mask, (f, m.group(0), txt[max(0, m.start() - 60):m.end() + 20])
            out.append((f, m.group(0), "UHC_EXP" if in_exp else "capi" if in_capi else "mask"))
    return out


def test_the_switch_scan_refuses_a_raw_bit_and_a_bare_name(tmp_path):
    """the scan above on two mutants of the sources: a numeric read of dbg in a kernel header, and a measurement switch's name outside UHC_EXP"""
    import shutil
    import pytest
    csrc = os.path.join(ROOT, "uhc_amd", "csrc")
    for k, (victim, old, new, said) in enumerate((("uhc_physics_impl.h", "A.dbg & UHC_DEBUG_NO_BOX_CULL", "A.dbg & 256", "dbg & 2"),
                                                  ("uhc_physics_impl.h", "UHC_EXP(UHC_DEBUG_EXP_NO_RANK_FILL)", "(A.dbg & UHC_DEBUG_EXP_NO_RANK_FILL)", "UHC_DEBUG_EXP_NO_RANK_FILL"))):
        d = tmp_path / str(k)
        shutil.copytree(csrc, d, ignore=shutil.ignore_patterns("build*", "*.so", "*.o"))
        txt = open(d / victim).read()
        assert txt.count(old) == 1
        open(d / victim, "w").write(txt.replace(old, new))
        with pytest.raises(AssertionError) as e:
            _switch_reads(str(d))
        assert victim in str(e.value) and said in str(e.value)


def test_product_package_never_imports_the_oracle():
    for d, _, files in os.walk(os.path.join(ROOT, "uhc_amd")):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(d, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, os.path.join(d, f)
    for f in os.listdir(os.path.join(ROOT, "uhc_amd", "csrc")):
        if f.endswith((".hip", ".cpp", ".h")):
            assert "oracle" not in open(os.path.join(ROOT, "uhc_amd", "csrc", f)).read().replace("the oracle", "").replace("and the oracle", ""), f
