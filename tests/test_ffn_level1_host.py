"""The one-product block tail (k_ffn128<., ., ., ., 1>: W_h X_h) and the automatic level's three-level rule.  No GPU.

  * the kernels this level must not touch -- every PROD == 2 and PROD == 3 instantiation of k_ffn128 and both k_attn_pw -- disassemble to the parent
    commit's instructions: tests/golden/ffn_level1_parent_isa.json holds, per kernel, the instruction count and the SHA-256 of the instruction stream
    (mnemonic and operands, one instruction per line, as tests/test_host.py's _disassemble_kernels returns them) of the library built from the parent
    commit with the same compiler; the shipped library must give the same digests.  `python tests/test_ffn_level1_host.py` prints that JSON for the
    library in the tree: a change that alters one of these kernels on purpose regenerates the file;
  * the new one-tile forms are pinned like level 2's: 256 + 256 registers, no SGPR spill, 768 MFMAs in the tail (512 + 256) plus 768 / 512 of the
    fused projection, level 2's ceilings for spilled VGPRs and scratch instructions, no scratch instruction inside GEMM 1's MFMA stream nor behind
    the projection's first MFMA;
  * the level rule (ffn_level_update in gn_api.hip, run through gn_debug_ffn_level_sim on synthetic flag arrays).
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.test_host import _disassemble_kernels  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "ffn_level1_parent_isa.json")
UNTOUCHED = ["k_ffn128ILi", "k_attn_pwILb"]


def _isa_digests(tmp_path):
    ks = _disassemble_kernels(tmp_path, UNTOUCHED)
    out = {}
    for name, (_, ins) in ks.items():
        if "k_ffn128" in name and name.split("EEEvNS")[0].endswith("ELi1"):       # the one-product forms: this level's own
            continue
        text = "\n".join(op + " " + ", ".join(args) for op, args in ins)
        out[name] = {"instructions": len(ins), "sha256": hashlib.sha256(text.encode()).hexdigest()}
    return out


def test_two_and_three_product_tails_and_bulk_attention_are_the_parents_instructions(tmp_path):
    with open(GOLDEN) as f:
        gold = json.load(f)["kernels"]
    have = _isa_digests(tmp_path)
    assert sum("k_attn_pwILb" in n and "ELi0EEEv" in n for n in gold) == 2 and sum("k_ffn128" in n and "ELi2EEEv" in n for n in gold) >= 6, sorted(gold)
    assert sorted(have) == sorted(gold), (sorted(set(have) ^ set(gold)))
    diff = [n for n in gold if have[n] != gold[n]]
    assert not diff, [(n, have[n]["instructions"], gold[n]["instructions"]) for n in diff]


def test_one_product_one_tile_forms_hold_their_registers(tmp_path):
    ks = _disassemble_kernels(tmp_path, ["k_ffn128ILi0ELb1ELb0ELi", "k_ffn128ILi8ELb1ELb0ELi0ELi1E", "k_ffn128ILi0ELb1ELb1ELi"])
    # (tag, MFMAs, of GEMM 1, of the tail, spilled VGPRs at most, scratch instructions at most): the ceilings are level 2's pins for the same form (test_host.py)
    for tag, nmf, n1, ntail, spills, scratch in (("k_ffn128ILi0ELb1ELb0ELi0ELi1E", 768, 512, 768, 4, 6), ("k_ffn128ILi0ELb1ELb0ELi1ELi1E", 1536, 512, 768, 4, 6),
                                                 ("k_ffn128ILi0ELb1ELb0ELi2ELi1E", 1280, 512, 768, 6, 8)):
        (name,) = [n for n in ks if tag in n]
        meta, ins = ks[name]
        assert meta["agpr_count"] == 256 and meta["vgpr_count"] == 512, meta
        assert meta["vgpr_spill_count"] <= spills and meta["sgpr_spill_count"] == 0, meta
        mf = [j for j, (op, _) in enumerate(ins) if op.startswith("v_mfma")]
        assert len(mf) == nmf, (name, len(mf))
        sc = [j for j, (op, _) in enumerate(ins) if op.startswith("scratch_")]
        assert len(sc) <= scratch, (name, len(sc))
        assert not any(mf[0] < j < mf[n1 - 1] for j in sc), (name, sc, mf[0], mf[n1 - 1])
        assert not any(j > mf[ntail] for j in sc if nmf > ntail), (name, sc)
        if nmf > ntail:     # the fused projection's epilogue stays scalar arithmetic, as on the other levels
            packed = [(j, op) for j, (op, _) in enumerate(ins) if j > mf[ntail] and op.startswith("v_pk_") and op.endswith("_f32")]
            assert not packed, (name, packed[:8])
    # the stamp form and the three walking forms exist, with the same MFMA counts
    for tag, nmf in (("k_ffn128ILi8ELb1ELb0ELi0ELi1E", 768), ("k_ffn128ILi0ELb1ELb1ELi0ELi1E", 768), ("k_ffn128ILi0ELb1ELb1ELi1ELi1E", 1536), ("k_ffn128ILi0ELb1ELb1ELi2ELi1E", 1280)):
        (name,) = [n for n in ks if tag in n]
        assert sum(op.startswith("v_mfma") for op, _ in ks[name][1]) == nmf and ks[name][0]["vgpr_count"] == 512, name


def _sim(f1, f2, f3, have1=True):
    """Run the rule over the calls of f_k[n_calls][B] (flags of level k's certificate); returns (levels of the calls, level after, switches, calls on one product)."""
    from gisnav_amd import _lib
    lib = _lib.load()
    f = [np.ascontiguousarray(a, np.int32) for a in (f1, f2, f3)]
    n, B = f[0].shape
    levels, out4 = np.zeros(n, np.int32), np.zeros(4, np.int64)
    rc = lib.gn_debug_ffn_level_sim(n, B, *(a.ctypes.data_as(C.c_void_p) for a in f), int(have1), levels.ctypes.data_as(C.c_void_p), out4.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return levels.tolist(), int(out4[0]), int(out4[1]), int(out4[3])


def _clean(n, B=16):
    return np.zeros((n, B), np.int32)


def test_128_clean_pairs_end_on_two_products_with_one_switch():
    z = _clean(8)
    levels, after, switches, calls1 = _sim(z, z, z)
    assert levels == [3, 3, 3, 3, 2, 2, 2, 2] and after == 2 and switches == 1 and calls1 == 0


def test_192_clean_pairs_end_on_one_product_with_two_switches():
    z = _clean(13)
    levels, after, switches, calls1 = _sim(z, z, z)
    assert levels == [3] * 4 + [2] * 8 + [1] and after == 1 and switches == 2 and calls1 == 1
    # without an eps for level 1 the rule is the two-level one
    levels, after, switches, _ = _sim(z, z, z, have1=False)
    assert levels == [3] * 4 + [2] * 9 and after == 2 and switches == 1


def test_two_consecutive_windows_are_needed_for_the_descent():
    # the second level-2 window flags 2 pairs in 64 on level 1 only: the run starts again, level 1 is reached two clean windows later
    z = _clean(20)
    f1 = z.copy()
    f1[8, 0] = f1[9, 3] = 1
    levels, after, switches, _ = _sim(f1, z, z)
    assert levels == [3] * 4 + [2] * 16 and after == 1 and switches == 2
    # one pair in 64 is tolerated
    f1 = z.copy()
    f1[8, 0] = 1
    levels, _, _, _ = _sim(f1, z, z)
    assert levels == [3] * 4 + [2] * 8 + [1] * 8


def test_a_failing_window_on_one_product_goes_back_to_two_or_to_three():
    z = _clean(20)
    f1 = z.copy()
    f1[12:16, :4] = 1                      # the first window on level 1: 16 of 64 flagged on level 1 only
    levels, after, switches, _ = _sim(f1, z, z)
    assert levels[12:16] == [1] * 4 and levels[16:] == [2] * 4 and switches == 3
    f2 = f1.copy()                          # ... and on level 2 as well: back to three products
    levels, after, switches, _ = _sim(f1, f2, z)
    assert levels[12:16] == [1] * 4 and levels[16:] == [3] * 4
    assert after == 2 and switches == 4          # (the clean window that follows on three products goes down to two again)
    # flags that level 3 raises too are no reason to leave (the re-run happens on every level)
    levels, after, _, _ = _sim(f1, f1, f1)
    assert levels[12:] == [1] * 8 and after == 1


def test_mid_margin_like_flags_never_leave_three_products():
    rng = np.random.default_rng(7)
    n, B = 24, 16
    f3 = (rng.random((n, B)) < 0.2).astype(np.int32)
    f2 = np.maximum(f3, (rng.random((n, B)) < 0.6).astype(np.int32))
    f1 = np.maximum(f2, (rng.random((n, B)) < 0.8).astype(np.int32))
    levels, after, switches, calls1 = _sim(f1, f2, f3)
    assert levels == [3] * n and after == 3 and switches == 0 and calls1 == 0


if __name__ == "__main__":
    import pathlib
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        from gisnav_amd import _lib
        print(json.dumps({"library_digest": _lib.library_digest(), "kernels": _isa_digests(pathlib.Path(d))}, indent=1, sort_keys=True))
