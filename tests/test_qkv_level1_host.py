"""The attention input projections on one fp16 product (W_h X_h: k_qkv<., true, 1> and k_ffn128<., ., ., 3 / 4, 1>) and the rung they add to the
automatic ladder below level 1.  No GPU.

  * the four new k_ffn128 forms (self / cross projection, one-tile / walking) disassemble to 768 + 384 = 1152 and 768 + 256 = 1024 MFMAs on 512 VGPRs + 256
    AGPRs, spill and use scratch no more than the two-product-projection forms <., ., ., 1 / 2, 1> of the same build, touch scratch neither inside GEMM 1 nor
    behind the tail (from the projection's first MFMA on), and keep the projection's epilogue scalar (no v_pk_*_f32 there);
  * k_qkv<., true, 1> has half the MFMAs of k_qkv<., true, 2>;
  * the level rule with the rung (ffn_level_next_rung in gn_api.hip, through gn_debug_ffn_level_sim_rung): 256 clean pairs end on the rung with three
    switches, 192 on level 1 with two, a failing window on the rung returns to level 1 (further when level 1 fails too), and without an eps for the rung every
    sequence of tests/test_ffn_level1_host.py gives gn_debug_ffn_level_sim's answer.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.test_ffn_level1_host import _clean, _sim  # noqa: E402
from tests.test_host import _disassemble_kernels  # noqa: E402

TAIL = 768      # MFMAs of the one-product tail (512 of GEMM 1 + 256 of GEMM 2)


@pytest.fixture(scope="module")
def tails(tmp_path_factory):
    return _disassemble_kernels(tmp_path_factory.mktemp("qkv_level1"), ["k_ffn128ILi0ELb1ELb0ELi", "k_ffn128ILi0ELb1ELb1ELi"])


def _one(ks, tag):
    (name,) = [n for n in ks if tag in n]
    return ks[name]


FORMS = [(loop, qkv, parent, nmf) for loop in (0, 1) for qkv, parent, nmf in ((3, 1, 1152), (4, 2, 1024))]


def _form(tails, loop, qkv):
    meta, ins = _one(tails, f"k_ffn128ILi0ELb1ELb{loop}ELi{qkv}ELi1E")
    return meta, ins, [j for j, (op, _) in enumerate(ins) if op.startswith("v_mfma")], [j for j, (op, _) in enumerate(ins) if op.startswith("scratch_")]


@pytest.mark.parametrize("loop,qkv,parent,nmf", FORMS)
def test_one_product_projection_forms_hold_their_registers(tails, loop, qkv, parent, nmf):
    meta, ins, mf, sc = _form(tails, loop, qkv)
    pmeta, pins, pmf, psc = _form(tails, loop, parent)
    assert meta["agpr_count"] == 256 and meta["vgpr_count"] == 512, meta
    assert len(mf) == nmf and len(pmf) == nmf + (384 if qkv == 3 else 256), (len(mf), len(pmf))
    print(f"loop {loop} qkv {qkv}: spilled VGPRs {meta['vgpr_spill_count']} (two-product projection {pmeta['vgpr_spill_count']}), SGPR spills {meta['sgpr_spill_count']} "
          f"({pmeta['sgpr_spill_count']}), scratch instructions {len(sc)} ({len(psc)}), instructions {len(ins)} ({len(pins)})")
    # spilled VGPRs and scratch instructions: no more than the two-product-projection form of the same build (the one-tile forms spill no SGPR, as every level's)
    assert meta["vgpr_spill_count"] <= pmeta["vgpr_spill_count"] and len(sc) <= len(psc), (meta, pmeta, len(sc), len(psc))
    assert loop == 1 or meta["sgpr_spill_count"] == 0, meta
    assert not any(mf[0] < j < mf[511] for j in sc), (sc, mf[0], mf[511])             # GEMM 1's MFMA stream
    assert not any(j > mf[TAIL] for j in sc), (sc, mf[TAIL])                             # the projection's k-loops and pass epilogues
    # (mf[TAIL]: the projection's first MFMA, the position tests/test_ffn_level1_host.py pins the two-product-projection forms at -- between the tail's last MFMA
    # and it lies the tail's own row-wise epilogue, which is packed f32 arithmetic by design and reloads one spilled value, in every form of every level)
    packed = [(j, op) for j, (op, _) in enumerate(ins) if j > mf[TAIL] and op.startswith("v_pk_") and op.endswith("_f32")]
    assert not packed, packed[:8]


def test_one_product_k_qkv_has_half_the_mfmas(tmp_path):
    ks = _disassemble_kernels(tmp_path, ["k_qkvILb"])
    for cross, two in ((0, 3 * 16 * 2 * 4), (1, 2 * 16 * 2 * 4)):      # passes x k-steps x products x token tiles
        n2 = sum(op.startswith("v_mfma") for op, _ in _one(ks, f"k_qkvILb{cross}ELb1ELi2E")[1])
        n1 = sum(op.startswith("v_mfma") for op, _ in _one(ks, f"k_qkvILb{cross}ELb1ELi1E")[1])
        assert n2 == two and 2 * n1 == n2, (cross, n1, n2)


def _sim_rung(f0, f1, f2, f3, have1=True, have0=True):
    """The rule with the rung over the calls of f_k[n_calls][B] (f0: the rung's flags); returns (levels of the calls, rung flags of the calls, level after, switches,
    calls on one product, on the rung after)."""
    from gisnav_amd import _lib
    lib = _lib.load()
    f = [np.ascontiguousarray(a, np.int32) for a in (f0, f1, f2, f3)]
    n, B = f[0].shape
    levels, rung, out5 = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(5, np.int64)
    rc = lib.gn_debug_ffn_level_sim_rung(n, B, *(a.ctypes.data_as(C.c_void_p) for a in f), int(have1), int(have0), levels.ctypes.data_as(C.c_void_p),
                                         rung.ctypes.data_as(C.c_void_p), out5.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return levels.tolist(), rung.tolist(), int(out5[0]), int(out5[1]), int(out5[3]), int(out5[4])


def test_256_clean_pairs_end_on_the_rung_with_three_switches_and_192_on_level_one_with_two():
    z = _clean(17)
    levels, rung, after, switches, calls1, on_rung = _sim_rung(z, z, z, z)
    assert levels == [3] * 4 + [2] * 8 + [1] * 5 and rung == [0] * 16 + [1], (levels, rung)
    assert after == 1 and on_rung == 1 and switches == 3 and calls1 == 5
    z = _clean(12)
    levels, rung, after, switches, _, on_rung = _sim_rung(z, z, z, z)
    assert levels == [3] * 4 + [2] * 8 and rung == [0] * 12 and after == 1 and on_rung == 0 and switches == 2
    # the rung needs level 1's window: one pair in 64 more than three products is tolerated, two are not
    z = _clean(20)
    f0 = z.copy()
    f0[12, 0] = 1
    assert _sim_rung(f0, z, z, z)[1] == [0] * 16 + [1] * 4
    f0[13, 5] = 1
    levels, rung, after, switches, _, on_rung = _sim_rung(f0, z, z, z)
    assert levels[12:] == [1] * 8 and rung == [0] * 20 and on_rung == 1 and switches == 3       # (the second level-1 window is clean: the rung after it)


def test_a_failing_window_on_the_rung_returns_to_level_one_or_further():
    z = _clean(28)
    f0 = z.copy()
    f0[16:20, :4] = 1                     # the first window on the rung: 16 of 64 flagged by the rung's certificate only
    levels, rung, after, switches, _, on_rung = _sim_rung(f0, z, z, z)
    assert levels[12:] == [1] * 16 and rung == [0] * 16 + [1] * 4 + [0] * 4 + [1] * 4, (levels, rung)       # back on level 1 for a window, clean there: the rung again
    assert switches == 5 and after == 1 and on_rung == 1
    levels, rung, after, switches, _, _ = _sim_rung(f0, f0, z, z)      # level 1's certificate flags them too: on to two products
    assert levels[16:20] == [1] * 4 and rung[16:20] == [1] * 4 and levels[20:24] == [2] * 4 and rung[20:] == [0] * 8, (levels, rung)
    levels, rung, _, _, _, _ = _sim_rung(f0, f0, f0, z)                # ... and level 2's: three products
    assert levels[20:24] == [3] * 4 and rung[20:] == [0] * 8
    # flags that three products raise as well are no reason to leave the rung
    levels, rung, after, _, _, on_rung = _sim_rung(f0, f0, f0, f0)
    assert levels[16:] == [1] * 12 and rung[16:] == [1] * 12 and on_rung == 1


def test_without_an_eps_for_the_rung_the_rule_is_the_three_level_one():
    rng = np.random.default_rng(11)
    seqs = []
    for n in (8, 13, 20, 24):
        seqs.append((_clean(n),) * 3)
    z = _clean(20)
    f1 = z.copy()
    f1[8, 0] = f1[9, 3] = 1
    seqs.append((f1, z, z))
    f1 = z.copy()
    f1[12:16, :4] = 1
    seqs += [(f1, z, z), (f1, f1, z), (f1, f1, f1)]
    f3 = (rng.random((24, 16)) < 0.2).astype(np.int32)
    f2 = np.maximum(f3, (rng.random((24, 16)) < 0.6).astype(np.int32))
    seqs.append((np.maximum(f2, (rng.random((24, 16)) < 0.8).astype(np.int32)), f2, f3))
    for f1, f2, f3 in seqs:
        for have1 in (True, False):
            want = _sim(f1, f2, f3, have1=have1)
            levels, rung, after, switches, calls1, on_rung = _sim_rung(np.ones_like(f1) - f1, f1, f2, f3, have1=have1, have0=False)
            assert (levels, after, switches, calls1) == want and not any(rung) and on_rung == 0
