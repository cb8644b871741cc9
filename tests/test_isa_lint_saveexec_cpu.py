"""CPU: tools/isa_lint.py and `s_or_saveexec_b64 sN, -1` -- EXEC | -1 switches every lane on, which is how the compiler reloads a VGPR that carries spilled SGPRs in
its lanes when that VGPR itself went to scratch.  Such a reload fills all 64 lanes, so a v_readlane of it is no hazard, wherever it executes; every other saveexec
around a reload still is one."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _lines(txt):
    return [(4 * k, l.strip()) for k, l in enumerate(txt.strip().splitlines())]


def test_reload_under_or_saveexec_all_lanes_then_readlane_is_no_hazard():
    import isa_lint
    # at the kernel's top level, and inside a divergent branch (the reload widens EXEC to all lanes, puts the branch's mask back, and the read runs in the branch)
    for txt in ("""
        s_or_saveexec_b64 s[10:11], -1
        scratch_load_dword v63, off, s32 offset:8
        s_mov_b64 exec, s[10:11]
        s_waitcnt vmcnt(0)
        v_readlane_b32 s6, v63, 40
    """, """
        v_cmp_gt_i32 vcc, 8, v0
        s_and_saveexec_b64 s[4:5], vcc
        s_or_saveexec_b64 s[10:11], -1
        scratch_load_dword v63, off, s32 offset:8
        s_mov_b64 exec, s[10:11]
        v_readlane_b32 s6, v63, 40
        s_or_b64 exec, exec, s[4:5]
        v_readlane_b32 s7, v63, 41
    """):
        haz, rev, st = isa_lint.lint_kernel("k", _lines(txt))
        assert not haz and not rev and st["scratch_loads"] == 1 and st["reloads_under_narrow_exec"] == 0, txt


def test_the_branch_mask_is_back_after_the_all_lanes_reload():
    import isa_lint
    # a SECOND reload, after EXEC was put back to the branch's mask, is a reload under a narrowed mask again
    haz, _, st = isa_lint.lint_kernel("k", _lines("""
        s_and_saveexec_b64 s[4:5], vcc
        s_or_saveexec_b64 s[10:11], -1
        scratch_load_dword v63, off, s32 offset:8
        s_mov_b64 exec, s[10:11]
        scratch_load_dword v7, off, s32 offset:16
        s_or_b64 exec, exec, s[4:5]
        v_readlane_b32 s6, v63, 40
        v_readlane_b32 s7, v7, 40
    """))
    assert [h[3] for h in haz] == ["v7"] and st["reloads_under_narrow_exec"] == 1


def test_reload_under_and_saveexec_then_readlane_after_the_restore_is_still_a_hazard():
    import isa_lint
    haz, rev, st = isa_lint.lint_kernel("k", _lines("""
        v_cmp_gt_i32 vcc, 8, v0
        s_and_saveexec_b64 s[4:5], vcc
        scratch_load_dword v63, off, s32 offset:8
        s_or_b64 exec, exec, s[4:5]
        v_readlane_b32 s6, v63, 40
    """))
    assert len(haz) == 1 and haz[0][3] == "v63" and not rev and st["reloads_under_narrow_exec"] == 1


def test_or_saveexec_with_a_mask_that_is_not_all_lanes_is_an_unknown_state():
    import isa_lint
    haz, _, st = isa_lint.lint_kernel("k", _lines("""
        s_or_saveexec_b64 s[10:11], s[12:13]
        scratch_load_dword v63, off, s32 offset:8
        s_mov_b64 exec, s[10:11]
        v_readlane_b32 s6, v63, 40
    """))
    assert len(haz) == 1 and st["reloads_under_narrow_exec"] == 1
