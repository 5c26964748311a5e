"""CPU checks of the drop-in boundary: the C-ABI library builds for gfx950, loads, and exports every
symbol include/lsm2d.h declares.  No compute calls here (no GPU in the build container)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "lsm2d.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lsm2d_[a-z0-9_]+)\s*\(", text)))


def test_library_builds_and_exports_every_declared_symbol():
    from srrg2_laser_slam_2d_amd import _capi, build
    path = build.build()
    assert os.path.exists(path)
    lib = C.CDLL(path)
    declared = _declared_symbols()
    assert len(declared) >= 15
    for name in declared:
        assert hasattr(lib, name), name
    bound = {s[0] for s in _capi.SYMBOLS}
    assert set(declared) == bound
    l = _capi.load()
    assert l.lsm2d_version() == 160
    assert l.lsm2d_status_string(0) == b"Success" and l.lsm2d_status_string(-4) == b"CapacityExceeded"


def test_no_silent_cpu_fallback():
    """Without a HIP device the product path must fail loudly, never compute on the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from srrg2_laser_slam_2d_amd import api
    with pytest.raises(api.Lsm2dError) as ei:
        api.Context(0)
    assert ei.value.code == -5


def test_product_package_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "srrg2_laser_slam_2d_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp")):
                src = open(os.path.join(dp, f)).read()
                assert "pyoracle" not in src and "lsm2d_oracle" not in src and "lsmo_" not in src, f


def test_struct_layouts_match_header_sizes():
    from srrg2_laser_slam_2d_amd import _capi
    assert C.sizeof(_capi.Projector) == 24
    assert C.sizeof(_capi.SliceParams) == 4 + 24 + 16 + 4 + 4 + 4 + 12 + 4 + 4
    assert C.sizeof(_capi.AlignerParams) == 24
    assert C.sizeof(_capi.Prior) == 48
    assert C.sizeof(_capi.Correspondence) == 8
    assert C.sizeof(_capi.IterationStats) == 28


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof / offsetof of every ABI struct as gcc lays include/lsm2d.h out, against the ctypes mirror field by field."""
    import subprocess
    from srrg2_laser_slam_2d_amd import _capi
    structs = {"lsm2d_projector": _capi.Projector, "lsm2d_slice_params": _capi.SliceParams, "lsm2d_aligner_params": _capi.AlignerParams,
               "lsm2d_prior": _capi.Prior, "lsm2d_correspondence": _capi.Correspondence, "lsm2d_iteration_stats": _capi.IterationStats,
               "lsm2d_preprocessor": _capi.Preprocessor, "lsm2d_batch": _capi.Batch}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lsm2d.h"', 'int main(void) {']
    for cname, st in structs.items():
        lines.append('printf("%s %%zu", sizeof(%s));' % (cname, cname))
        for fname, _ in st._fields_:
            lines.append('printf(" %s=%%zu", offsetof(%s, %s));' % (fname, cname, fname))
        lines.append('printf("\\n");')
    lines += ['return 0; }']
    src = tmp_path / "layout.c"; src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    for line in out.strip().splitlines():
        parts = line.split(); st = structs[parts[0]]
        assert int(parts[1]) == C.sizeof(st), (parts[0], parts[1], C.sizeof(st))
        for kv in parts[2:]:
            k, v = kv.split("=")
            assert getattr(st, k).offset == int(v), (parts[0], k, v, getattr(st, k).offset)


def test_adapters_use_no_shim_only_member():
    """The stand-in headers imitate Eigen's and srrg2's PUBLIC surface; what is theirs alone is private or carries `shim` in its name.  An
    adapter that compiles against them can still only be trusted if it never names such a thing (round 2's raw-data preprocessor wrote
    `sensor_matrix.m[0][0]`, a member of the stand-in, where Eigen wants `sensor_matrix << ...`)."""
    ad = os.path.join(ROOT, "adapters", "srrg")
    for f in sorted(os.listdir(ad)):
        text = re.sub(r"//.*", "", open(os.path.join(ad, f)).read())
        assert not re.search(r"shim", text, re.I), f
        assert not re.search(r"\.\s*(m|v)\s*\[", text), (f, "raw storage of a stand-in matrix / vector")
        assert not re.search(r"\._(c|s|tx|ty|m|v|props)\b", text), (f, "private storage of a stand-in type")
    # and the one place where Eigen's comma initialiser is needed uses it, as the reference does (raw_data_preprocessor_projective_2d.cpp:89-90)
    assert "sensor_matrix <<" in open(os.path.join(ad, "raw_data_preprocessor_hip_2d.h")).read()


def test_srrg_adapter_sources_compile_against_the_stand_in_headers(tmp_path):
    """adapters/srrg/* are written against the srrg2 stack, which is absent from this image.  tests/cpp/adapter_shim holds stand-in
    headers (test infrastructure) declaring exactly the upstream names those sources use, so every adapter translation unit -- and the
    driver the GPU test runs -- is at least COMPILED here (g++, no GPU needed)."""
    import cpp_build
    inc = [os.path.join(ROOT, "adapters", "srrg"), os.path.join(ROOT, "tests", "cpp", "adapter_shim")]
    units = [os.path.join(ROOT, "adapters", "srrg", "correspondence_finder_hip_2d.cpp"), os.path.join(ROOT, "adapters", "srrg", "multi_aligner_hip_2d.cpp"),
             os.path.join(ROOT, "tests", "cpp", "adapter_driver.cpp")]      # the driver includes mapping_hip_2d.h and raw_data_preprocessor_hip_2d.h (header-only)
    for u in units:
        r = cpp_build.syntax_only(u, include_dirs=inc)
        assert r.returncode == 0, r.stderr[-3000:]
    # every entry point the adapters call is declared in include/lsm2d.h and exported by the library
    import re
    used = set()
    for dp, _, files in os.walk(os.path.join(ROOT, "adapters", "srrg")):
        for f in files:
            used |= set(re.findall(r"\b(lsm2d_[a-z_0-9]+)\s*\(", open(os.path.join(dp, f)).read()))
    declared = set(_declared_symbols())
    assert used and used <= declared, used - declared


# ---- the adapters' and the compile shim's PARAMs against the reference's own headers ------------------------------------------
# (the reference's side is tests/golden/reference_params.json, read out of its headers and sources by tests/golden/make_reference_params.py)
REFERENCE_CLASSES = [("registration/correspondence_finder_projective_2d.h", "CorrespondenceFinderProjective2f"),
                     ("registration/correspondence_finder_kd_tree_2d.h", "CorrespondenceFinderKDTree2D"),
                     ("registration/correspondence_finder_nn_2d.h", "CorrespondenceFinderNN2D"),
                     ("mapping/scene_clipper_projective_2d.h", "SceneClipperProjective2D"),
                     ("mapping/merger_projective_2d.h", "MergerProjective2D"),
                     ("sensor_processing/raw_data_preprocessor_projective_2d.h", "RawDataPreprocessorProjective2D")]


def _reference():
    import json
    from conftest import golden_path
    return json.load(open(golden_path("reference_params.json")))


def _reference_params(header, class_name):
    ent = _reference()["params"][class_name]
    assert ent["header"] == header, (class_name, ent["header"], header)
    return {name: tuple(v) for name, v in ent["params"].items()}


def _params_of(text, class_name):
    """(type, name, default) of every PARAM(...) inside `class class_name`; nesting-aware split, `srrg2_core::` stripped."""
    import re
    m = re.search(r"class\s+" + class_name + r"\b[^;{]*\{", text)
    if not m:
        return None
    depth, i = 1, m.end()
    while depth and i < len(text):
        depth += {"{": 1, "}": -1}.get(text[i], 0); i += 1
    body = text[m.end():i]
    out = {}
    for pm in re.finditer(r"\bPARAM\s*\(", body):
        j, d, fields, cur, in_str = pm.end(), 1, [], "", False
        while d and j < len(body):
            ch = body[j]
            if ch == '"' and body[j - 1] != "\\":
                in_str = not in_str
            if not in_str:
                if ch in "(<":
                    d += 1
                elif ch in ")>":
                    d -= 1
                    if d == 0:
                        break
                elif ch == "," and d == 1:
                    fields.append(cur.strip()); cur = ""; j += 1
                    continue
            cur += ch; j += 1
        fields.append(cur.strip())
        typ, name, default = fields[0].replace("srrg2_core::", "").replace(" ", ""), fields[1], fields[3]
        try:
            default = float(default.rstrip("fF")) if not default.endswith(")") else "expr"
        except ValueError:
            default = "expr"
        out[name] = (typ, default)
    return out


def test_adapter_and_shim_params_match_the_reference_headers():
    """Every PARAM the reference declares for the classes the adapters replace or recognise (tests/golden/reference_params.json) exists,
    with the same property type and default, in (a) the stand-in headers the adapters are compile-checked against and (b) the adapters'
    own sibling classes -- a configuration written for the reference loads unchanged."""
    rd = lambda *p: open(os.path.join(*p)).read()
    shim = rd(ROOT, "tests", "cpp", "adapter_shim", "srrg_shim.h")
    fh = rd(ROOT, "adapters", "srrg", "correspondence_finder_hip_2d.h"); mh = rd(ROOT, "adapters", "srrg", "mapping_hip_2d.h")
    cases = [("registration/correspondence_finder_projective_2d.h", "CorrespondenceFinderProjective2f", shim, fh, "CorrespondenceFinderHIP2D"),
             ("registration/correspondence_finder_kd_tree_2d.h", "CorrespondenceFinderKDTree2D", shim, fh, "CorrespondenceFinderKDTreeHIP2D"),
             ("registration/correspondence_finder_nn_2d.h", "CorrespondenceFinderNN2D", shim, fh, "CorrespondenceFinderNNHIP2D"),
             ("mapping/scene_clipper_projective_2d.h", "SceneClipperProjective2D", None, mh, "SceneClipperHIP2D"),
             ("mapping/merger_projective_2d.h", "MergerProjective2D", None, mh, "MergerHIP2D"),
             ("sensor_processing/raw_data_preprocessor_projective_2d.h", "RawDataPreprocessorProjective2D", None,
              rd(ROOT, "adapters", "srrg", "raw_data_preprocessor_hip_2d.h"), "RawDataPreprocessorHIP2D")]
    for header, cls, shim_text, adapter_text, adapter_cls in cases:
        want = _reference_params(header, cls)
        assert want, (header, cls)
        for where, text, name in (("shim", shim_text, cls), ("adapter", adapter_text, adapter_cls)):
            if text is None:
                continue
            got = _params_of(text, name)
            assert got is not None, (where, name)
            for pname, (typ, default) in want.items():
                assert pname in got, (where, name, "missing PARAM", pname)
                assert got[pname][0] == typ, (where, name, pname, got[pname][0], typ)
                if default != "expr":
                    assert got[pname][1] == "expr" or abs(got[pname][1] - default) <= 1e-6 * max(1.0, abs(default)), (where, name, pname, got[pname][1], default)


def test_python_mirror_defaults_match_the_reference_headers():
    """The Python mirror of the reference classes (srrg2_laser_slam_2d_amd/api.py) takes the reference's PARAM names as keyword arguments:
    every numeric default must be the reference's (tests/golden/reference_params.json)."""
    import inspect
    from srrg2_laser_slam_2d_amd import api
    cases = [("registration/correspondence_finder_projective_2d.h", "CorrespondenceFinderProjective2f", api.CorrespondenceFinderProjective2f),
             ("registration/correspondence_finder_kd_tree_2d.h", "CorrespondenceFinderKDTree2D", api.CorrespondenceFinderKDTree2D),
             ("registration/correspondence_finder_nn_2d.h", "CorrespondenceFinderNN2D", api.CorrespondenceFinderNN2D),
             ("mapping/scene_clipper_projective_2d.h", "SceneClipperProjective2D", api.SceneClipperProjective2D),
             ("mapping/merger_projective_2d.h", "MergerProjective2D", api.MergerProjective2D),
             ("sensor_processing/raw_data_preprocessor_projective_2d.h", "RawDataPreprocessorProjective2D", api.RawDataPreprocessorProjective2D)]
    checked = 0
    for header, cls, mirror in cases:
        want = _reference_params(header, cls)
        sig = inspect.signature(mirror.__init__).parameters
        for pname, (typ, default) in want.items():
            if default == "expr" or typ == "PropertyString":
                continue                                     # object-valued (projector, un-projector, normal computator) / topic strings: not numeric
            assert pname in sig, (cls, "mirror lacks", pname)
            assert abs(float(sig[pname].default) - default) <= 1e-6 * max(1.0, abs(default)), (cls, pname, sig[pname].default, default)
            checked += 1
    assert checked >= 12


def test_adapters_touch_only_base_class_members_the_reference_uses():
    """The adapters derive from upstream base classes this image does not have; the members they read and write there (`_fixed`,
    `_full_scene`, `_meas`, ...) are the ones the reference's own implementations of the same classes use: every underscore-member an
    adapter touches is either declared by the adapter itself, used somewhere in the reference's sources (tests/golden/reference_params.json,
    member_ids), or one of the names isolated (and tagged UPSTREAM) in adapters/srrg/upstream_access.h / multi_aligner_hip_2d.cpp."""
    ref_ids = set(_reference()["member_ids"])
    upstream_tagged = {"_fixed_slice", "_moving_slice", "_information_matrix", "_iteration_stats"}     # upstream_access.h:58-68, multi_aligner_hip_2d.cpp (_writeBack)
    ad = os.path.join(ROOT, "adapters", "srrg")
    texts = {f: re.sub(r"//.*", "", open(os.path.join(ad, f)).read()) for f in sorted(os.listdir(ad))}
    own = set()
    for t in texts.values():       # members, methods and locals the adapters declare themselves
        own |= set(re.findall(r"[\w>\*&\]]\s+\**(_[a-z][a-zA-Z_0-9]*)\s*(?:=|;|\{|\[|,|\()", t))
        for decl in re.findall(r"^\s*[\w:<>\*&, ]+?\s+\**(_[a-z][a-zA-Z_0-9]*(?:\s*(?:=[^,;]*)?,\s*\**_[a-z][a-zA-Z_0-9]*)+)\s*(?:=[^;]*)?;", t, re.M):
            own |= set(re.findall(r"_[a-z][a-zA-Z_0-9]*", decl))              # "Type _a, _b;" declares both
    seen_base = set()
    for f, t in texts.items():
        for name in set(re.findall(r"\b_[a-z][a-zA-Z_0-9]*\b", t)):
            if name.endswith("_") or name in own:
                continue
            assert name in ref_ids or name in upstream_tagged, (f, name)
            seen_base.add(name)
    assert {"_fixed", "_moving", "_correspondences", "_local_map_in_sensor", "_full_scene", "_clipped_scene_in_robot", "_scene", "_measurement",
            "_measurement_in_scene", "_robot_in_local_map", "_sensor_in_robot", "_meas", "_raw_data", "_status"} <= seen_base
