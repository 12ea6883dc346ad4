"""CPU-side tests of the split-fp16 attention mode (GN_PREC_F16X2_F16X2_ATTN = 5) and the certificate's re-run ladder: the Python surface, the
binding of the new entry points, and the shipped k_attn_f16x2 code.  No GPU compute here."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def _header_enum(name):
    hdr = open(os.path.join(ROOT, "include", "gisnav_amd.h")).read()
    m = re.search(rf"\b{name}\s*=\s*(\d+)", hdr)
    assert m, name
    return int(m.group(1))


def test_mode5_is_a_precision_of_the_python_surface():
    from gisnav_amd import _lib
    from gisnav_amd.engine import _PRECISIONS
    assert "f16x2_f16x2_attn" in _PRECISIONS
    assert _PRECISIONS["f16x2_f16x2_attn"] == _lib.GN_PREC_F16X2_F16X2_ATTN == _header_enum("GN_PREC_F16X2_F16X2_ATTN") == 5


def test_ladder_entry_points_are_declared_and_bound():
    from gisnav_amd import build, _lib
    build.build(verbose=False)
    hdr = open(os.path.join(ROOT, "include", "gisnav_amd.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gn_set_certify_ladder", "gn_get_certify_ladder_stats"):
        assert re.search(rf"\bint {name}\(", hdr), name
        assert name in _lib.SIGNATURES
        assert hasattr(raw, name)
    assert _lib.SIGNATURES["gn_set_certify_ladder"][1][1:] == [ctypes.c_int, ctypes.c_float]


def test_ladder_refused_where_there_is_nothing_to_ladder():
    from gisnav_amd.matcher import LightGlueMatcher
    p = {"depth_confidence": -1, "width_confidence": -1}
    with pytest.raises(ValueError):
        LightGlueMatcher("sift", params=p, state_dict={}, precision="f32", certify_ladder=True)
    with pytest.raises(ValueError):
        LightGlueMatcher("sift", params=p, state_dict={}, precision="f16x2_f16x2_attn", certify_ladder=True)
    with pytest.raises(ValueError):
        LightGlueMatcher("sift", params=p, state_dict={}, precision="f16x2_f16_attn", certify=False, certify_ladder=True)
    m = LightGlueMatcher("sift", params=p, state_dict={}, precision="f16x2_f16_attn", certify_ladder=True)
    assert m._ladder is True


def test_ladder_keyword_defaults_to_off():
    import inspect
    from gisnav_amd.matcher import LightGlueMatcher
    from gisnav_amd.pose_node import PoseNode
    for cls in (LightGlueMatcher, PoseNode):
        prm = inspect.signature(cls.__init__).parameters["certify_ladder"]
        assert prm.default is False and prm.kind is inspect.Parameter.KEYWORD_ONLY, cls
    m = LightGlueMatcher("sift", params={"depth_confidence": -1, "width_confidence": -1}, state_dict={}, precision="f16x2_f16_attn")
    assert m._ladder is False


def _kernel_code(tmp_path, wanted):
    """{mangled name: (metadata, disassembly text)} of the shipped library's kernels whose name contains `wanted`."""
    from gisnav_amd import build
    build.build(verbose=False)
    assert os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/llvm-readelf")
    so = shutil.copy(os.path.join(ROOT, "gisnav_amd", "libgisnav_amd.so"), tmp_path / "lib.so")
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", os.path.basename(so)], cwd=tmp_path, check=True, capture_output=True)
    out = {}
    for f in sorted(f for f in os.listdir(tmp_path) if "hipv4" in f):
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", f], cwd=tmp_path, check=True, capture_output=True, text=True).stdout
        if wanted not in notes:
            continue
        meta = {}
        for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            kv = dict(re.findall(r"\.(name|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s*(\S+)", blk))
            if "name" in kv:
                meta[kv["name"]] = kv
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", f], cwd=tmp_path, check=True, capture_output=True, text=True).stdout
        parts = re.split(r"\n[0-9a-f]+ <([^>]+)>:\n", dis)
        for i in range(1, len(parts), 2):
            if wanted in parts[i] and parts[i] in meta:
                out[parts[i]] = (meta[parts[i]], parts[i + 1])
    return out


def test_shipped_attn_f16x2_is_split_fp16_on_the_16bit_pipe(tmp_path):
    code = _kernel_code(tmp_path, "k_attn_f16x2")
    assert len(code) == 2, sorted(code)              # the bulk form and the key-split form
    for name, (meta, dis) in code.items():
        assert dis.count("v_mfma_f32_32x32x16_f16") >= 24, name         # 12 per 32-key tile for S, 12 for O (three products each)
        assert "v_mfma_f32_32x32x2_f32" not in dis, name
        assert not re.search(r"\b(scratch|buffer)_(load|store)", dis), name
        assert int(meta.get("private_segment_fixed_size", 0)) == 0, name
        assert int(meta.get("vgpr_spill_count", 0)) == 0 and int(meta.get("sgpr_spill_count", 0)) == 0, name
        for m in re.finditer(r"v_pk_fma_f32 (.*)", dis):
            sel = re.search(r"op_sel:\[([01]),([01]),([01])\]", m.group(1))
            assert not (sel and "1" in sel.groups()), (name, m.group(0))
