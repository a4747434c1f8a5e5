"""The multi-map (rebuild) kernels are a build-ID family of their own
(erasure_coding_test_amd/build.py KERNEL_FAMILIES, ecgpu_build_id(5)): an edit
to a maps file changes the library's ID and the rebuild ID only, and an edit
to another family's kernels leaves the rebuild ID -- which
profiles/rebuild.json is keyed to -- alone.  CPU only.
"""
import ctypes

from test_build import LIB, _build_module, _ids_with_edit

MAPS_FILES = ("maps_kernels.hpp", "maps_spec.hip", "maps_spec.hpp", "maps.hip")
OTHER_FAMILIES = ("kernels", "wide", "packets", "scrub")


def test_library_reports_the_rebuild_id():
    b = _build_module()
    lib = ctypes.CDLL(LIB)
    lib.ecgpu_build_id.restype = ctypes.c_char_p
    lib.ecgpu_build_id.argtypes = [ctypes.c_int]
    ids = b.build_ids()
    assert lib.ecgpu_build_id(5).decode() == ids["rebuild"], "libecgpu.so is stale: rebuild"
    assert lib.ecgpu_build_id(4).decode() == ids["scrub"]
    assert len(ids["rebuild"]) == 16 and len({ids[f] for f in OTHER_FAMILIES + ("rebuild", "build")}) == 6


def test_maps_units_are_built_once_per_row_count():
    b = _build_module()
    units = [(src, obj, extra) for src, obj, extra in b.HIP_UNITS if src.startswith("maps")]
    assert sorted(u[0] for u in units) == ["maps.hip"] + ["maps_spec.hip"] * 4
    assert sorted(e for u in units for e in u[2]) == [f"-DECGPU_SPEC_R={r}" for r in (1, 2, 3, 4)]
    assert len({u[1] for u in units}) == 5


def test_a_maps_edit_changes_build_and_rebuild_only(tmp_path):
    b = _build_module()
    base = b.build_ids()
    for name in MAPS_FILES:
        ids = _ids_with_edit(b, tmp_path, name)
        assert ids["rebuild"] != base["rebuild"] and ids["build"] != base["build"], name
        assert all(ids[f] == base[f] for f in OTHER_FAMILIES), (name, ids, base)


def test_other_families_edits_leave_the_rebuild_id(tmp_path):
    b = _build_module()
    base = b.build_ids()
    for name in ("gf_kernels_w8.hpp", "gf_spec.hip", "dispatch_w8.hip", "residency_w8.hpp", "gf_kernels_wide.hpp",
                 "wide_spec.hip", "dispatch_wide.hip", "gf_kernels_packets.hpp", "packets.hip", "scrub_kernels.hpp",
                 "scrub_spec.hip", "scrub.hip", "plans.hip", "diag_kernels_w8.hpp"):
        assert _ids_with_edit(b, tmp_path, name)["rebuild"] == base["rebuild"], name
    # the device vocabulary is in every family
    assert _ids_with_edit(b, tmp_path, "gf_device.hpp")["rebuild"] != base["rebuild"]
    # the dispatch reads the cap and store-policy knobs, not the scrub's or the engine's
    cap = _ids_with_edit(b, tmp_path, "knobs.cpp", ('{"ECGPU_CAP", "cap", -1}', '{"ECGPU_CAP", "cap", 1}'))
    assert cap["rebuild"] != base["rebuild"]
    pipe = _ids_with_edit(b, tmp_path, "knobs.cpp", ('{"ECGPU_WIDE_PIPE", "wide_pipe", 1}',
                                                     '{"ECGPU_WIDE_PIPE", "wide_pipe", 2}'))
    assert pipe["rebuild"] == base["rebuild"]


def test_committed_rebuild_record_carries_the_rebuild_build_id():
    import json
    import os
    import re
    from test_build import ROOT
    with open(os.path.join(ROOT, "profiles", "rebuild.json")) as f:
        d = json.load(f)
    assert re.fullmatch(r"[0-9a-f]{16}", d["ecgpu_build_id"]) and d["ecgpu_build_id"] == d["build_ids"]["rebuild"]
    assert d["rounds"] == 20 and d["reps_per_round"] == 5
    for shape, stripes, patterns in (("S1", 96, 14), ("S2", 1365, 91)):
        s = d["shapes"][shape]
        assert (s["shape"]["stripes"], s["shape"]["patterns"]) == (stripes, patterns)
        assert set(s["arms"]) == {"A", "B", "C"} and set(s["create_and_bind_host_ms"]) == {"A", "B"}
        assert isinstance(s["expectation"]["a_within_b_spread"], bool)
