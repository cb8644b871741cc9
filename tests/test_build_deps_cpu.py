"""CPU (needs hipcc, like tests/test_capi_symbols.py): what an object of libuhc_amd.so is cached under.  __graft_entry__.unit_deps asks the compiler which files of
the repository a translation unit includes; unit_key hashes the source, those files and the flags.  A header that is split off or added needs no entry in any table --
these tests say what must come out of that: no header is left out, the env layer and the step kernels stay apart, and an edit of a header changes the key of
exactly the units that include it."""
import os
import shutil
from concurrent.futures import ThreadPoolExecutor

import pytest

import __graft_entry__ as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uhc_amd", "csrc")
STEP_UNITS = [s for s in g.HIP_SOURCES if s.startswith("uhc_k_")] + ["uhc_batch_kernels.hip"]  # the units that include uhc_physics_impl.h
ENV_UNITS = ["uhc_env.hip", "uhc_env_capi.cpp", "uhc_expert.hip"]
STEP_HEADERS = ["uhc_physics_impl.h", "uhc_mpr.h", "uhc_primal.h", "uhc_device.h", "uhc_step_words.h", "uhc_launch.h"]
POST_UNITS = ["uhc_expert.hip", "uhc_eval.hip", "uhc_smpl.hip", "uhc_surface.hip", "uhc_smpl_mesh.hip", "uhc_rollout.hip", "uhc_live.hip"]  # the device-side post-processing
POST_HEADERS = ["uhc_seq.h", "uhc_api_check.h"]  # their shared sequence rules and host-side checks
TIER4_UNITS =["uhc_k_big.hip", "uhc_k_big_fwd.hip", "uhc_k_huge_q.hip"]  # (#define UHC_WITH_TIER4: tier 4 is compiled into the large tier's kernels only)


@pytest.fixture(scope="module")
def deps():
    """{unit: the names of its dependencies inside csrc} + the full paths, for every unit of the library at the shipped flags"""
    full = {s: g.unit_deps(s, g.unit_flags()) for s in g.HIP_SOURCES}
    return {s: {os.path.basename(f) for f in d if os.path.dirname(f) == CSRC} for s, d in full.items()}, full


def test_every_unit_is_listed_and_every_header_is_somebodys_dependency(deps):
    names, _ = deps
    on_disk = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp")))
    assert on_disk == sorted(g.HIP_SOURCES)
    headers = {f for f in os.listdir(CSRC) if f.endswith(".h")}
    used = set().union(*names.values())
    assert headers - used == set(), "orphan headers"
    assert set(STEP_HEADERS) <= headers


def test_step_units_depend_on_the_step_headers(deps):
    names, _ = deps
    assert len(STEP_UNITS) == 12
    for u in STEP_UNITS:
        assert {"uhc_physics_impl.h", "uhc_mpr.h", "uhc_device.h", "uhc_step_words.h"} <= names[u], u
        assert ("uhc_launch.h" in names[u]) == u.startswith("uhc_k_"), u  # (the launch table: every kernel unit, not the batch kernels)
        assert ("uhc_primal.h" in names[u]) == (u in TIER4_UNITS), u


def test_env_layer_depends_on_no_step_header(deps):
    names, _ = deps
    for u in ENV_UNITS:
        assert names[u] & set(STEP_HEADERS) == set(), (u, names[u])
        assert "uhc_device_env.h" in names[u]
    assert names["uhc_rollout.hip"] == {"uhc_api_check.h"}


def test_post_processing_units_and_step_units_stay_apart(deps):
    # the post-processing units read no step header (an edit of the step does not rebuild them), and no step unit reads the two headers those units share
    # (an edit of uhc_seq.h or uhc_api_check.h rebuilds no step-kernel object)
    names, _ = deps
    for u in POST_UNITS:
        assert names[u] & set(STEP_HEADERS) == set(), (u, names[u])
        # (uhc_rollout.hip has no sequences, uhc_live.hip -- its model index clamped by the same rule -- no C entry of its own)
        assert ("uhc_seq.h" in names[u]) == (u != "uhc_rollout.hip") and ("uhc_api_check.h" in names[u]) == (u != "uhc_live.hip"), (u, names[u])
    for u in STEP_UNITS:
        assert names[u] & set(POST_HEADERS) == set(), (u, names[u])


def test_the_internal_seams_header_is_read_by_the_units_on_either_side_of_a_seam_and_no_other(deps):
    # uhc_internal.h declares the launchers and accessors the units share: the units that DEFINE one (the three kernel units, uhc_capi.cpp) and the two that CALL
    # them read it, so a prototype cannot differ between them; no step-kernel unit does (an edit of it rebuilds none of their objects, ~4 minutes), and nothing
    # the step kernels include pulls it in
    names, _ = deps
    seams = {"uhc_batch_kernels.hip", "uhc_env.hip", "uhc_live.hip", "uhc_capi.cpp", "uhc_env_capi.cpp"}
    assert {u for u in g.HIP_SOURCES if "uhc_internal.h" in names[u]} == seams
    assert not any(u.startswith("uhc_k_") for u in seams)
    for h in ("uhc_launch.h", "uhc_physics_impl.h", "uhc_device.h", "uhc_api_check.h", "uhc_device_env.h"):
        assert '#include "uhc_internal.h"' not in open(os.path.join(CSRC, h)).read(), h
    # the env's plan (and the struct of the batch's dims beside it): the unit that fills the struct and the unit that plans from it
    assert {u for u in g.HIP_SOURCES if "uhc_env_plan.h" in names[u]} == {"uhc_capi.cpp", "uhc_env_capi.cpp"}
    # uhc_internal_set_error's one declaration: its definer reads it too
    assert "uhc_api_check.h" in names["uhc_capi.cpp"]


def test_every_dependency_lies_inside_the_repository(deps):
    _, full = deps
    for u, d in full.items():
        assert d, u  # (every unit includes at least include/uhc_amd.h or the env layer's header)
        for f in d:
            assert os.path.isabs(f) and os.path.realpath(f).startswith(os.path.realpath(ROOT) + os.sep) and os.path.isfile(f), (u, f)
            assert f != os.path.join(CSRC, u)


def test_flags_select_the_dependencies_and_enter_the_key():
    # -D flags reach the preprocessor that lists the dependencies: without UHC_WITH_TIER4 (which the unit defines itself) no unit reads uhc_primal.h, with it on the command line one does
    assert "uhc_primal.h" in {os.path.basename(f) for f in g.unit_deps("uhc_k_general.hip", g.unit_flags(["-DUHC_WITH_TIER4"]))}
    assert g.unit_key("uhc_env.hip", g.unit_flags()) != g.unit_key("uhc_env.hip", g.unit_flags(["-DUHC_STAGE_PROF"]))
    assert g.unit_key("uhc_env.hip", g.unit_flags()) == g.unit_key("uhc_env.hip", g.unit_flags())


def test_an_edit_changes_the_keys_of_exactly_the_units_that_include_the_file(tmp_path, deps):
    names, _ = deps
    csrc = tmp_path / "uhc_amd" / "csrc"
    csrc.mkdir(parents=True)
    for f in os.listdir(CSRC):
        if f.endswith((".h", ".hip", ".cpp")):
            shutil.copy(os.path.join(CSRC, f), csrc / f)
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    flags = g.unit_flags()

    def keys(where=str(csrc)):
        with ThreadPoolExecutor(8) as pool:
            return dict(zip(g.HIP_SOURCES, pool.map(lambda s: g.unit_key(s, flags, where), g.HIP_SOURCES)))

    # the copy's dependencies are the copy's files: nothing of the key reaches back into this tree
    for s in ("uhc_k_big.hip", "uhc_capi.cpp", "uhc_env.hip"):
        assert all(f.startswith(str(tmp_path.resolve()) + os.sep) for f in g.unit_deps(s, flags, str(csrc)))
    before = keys()
    assert before == keys(CSRC)  # (same contents, same flags: same keys)
    for edited in ("uhc_mpr.h", "uhc_primal.h", "uhc_device_env.h", "uhc_env.hip", "uhc_internal.h"):
        with open(csrc / edited, "a") as f:
            f.write("// an edit\n")
        after = keys()
        changed = {s for s in g.HIP_SOURCES if after[s] != before[s]}
        assert changed == {s for s in g.HIP_SOURCES if edited in names[s] or s == edited}, edited
        assert changed, edited
        before = after
    with open(tmp_path / "include" / "uhc_amd.h", "a") as f:
        f.write("/* an edit */\n")
    after = keys()
    assert {s for s in g.HIP_SOURCES if after[s] != before[s]} == set(g.HIP_SOURCES) - {"uhc_env.hip"}  # (the one unit that does not read the public header)
