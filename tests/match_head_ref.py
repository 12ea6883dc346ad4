"""NumPy fp64 reference of the match head (csrc/gn_match_head.hip), shared by tests/test_match_head_host.py and tests/test_gpu_match_head.py.

The head turns projected descriptors md [2][n][256], log-sigmoid matchabilities ls [2][n] and a threshold th into

    S = md0 . md1^T
    P = log_softmax(S, rows) + log_softmax(S, cols) + ls0_i + ls1_j          (kornia's sigmoid_log_double_softmax without the dustbins)
    best / runner-up (multiplicity counted: an exact tie has runner-up == best) / arg-max (lowest index) of every row and column of P
    the filter_matches list: (i, m0[i]) for rows with m1[m0[i]] == i and exp(best_i) > th, in row order
    the margin certificate's three verdicts (rule)

Two operand models (similarity): "f32" contexts multiply the f32 descriptors; "f16x2" contexts multiply what k_split_hm16 makes of them,
h = float16(x), m = float16(x - h), S = A_h B_h^T + A_h B_m^T + A_m B_h^T (the A_m B_m^T term is dropped by the kernel, so it is dropped here).

Everything a GPU assertion depends on -- inputs, cases, tie positions, the eps / threshold table -- is built here from seeds and from fp64 values
alone, so that the host test can assert the cases' preconditions without a GPU.
"""
import functools
import math

import numpy as np

FORMATS = ("f32", "f16x2")
BUDGET_FACTOR = 4.0      # a stage's distance from fp64 may be 4 x the distance of an f32 NumPy evaluation of the same formula on the same operands


# ------------------------------------------------------------------------------------------------ inputs
def logsigmoid(z):
    return -np.logaddexp(0.0, -z)


def make_inputs(seed, npad, nvalid, padding="garbage"):
    """md [B][2][npad][256] ~ N(0, 0.5^2), ls [B][2][npad] = logsigmoid(N(2, 3^2)), nvalid [B][2]; rows at and beyond nvalid hold finite garbage
    (|x| <= 1e4) or zeros.  The valid part does not depend on `padding`."""
    nv = np.asarray(nvalid, np.int32).reshape(-1, 2)
    B = nv.shape[0]
    rng = np.random.default_rng(seed)
    md = rng.normal(0.0, 0.5, (B, 2, npad, 256)).astype(np.float32)
    ls = logsigmoid(rng.normal(2.0, 3.0, (B, 2, npad))).astype(np.float32)
    pad = np.arange(npad)[None, None, :] >= nv[:, :, None]
    g_md = rng.uniform(-1.0e4, 1.0e4, md.shape).astype(np.float32)
    g_ls = rng.uniform(-1.0e4, 1.0e4, ls.shape).astype(np.float32)
    md[pad] = g_md[pad] if padding == "garbage" else 0.0
    ls[pad] = g_ls[pad] if padding == "garbage" else 0.0
    return dict(md=md, ls=ls, nvalid=nv, npad=npad, B=B)


def swap_sides(inp):
    """The same pairs with image 0 and image 1 exchanged: P becomes its transpose."""
    return dict(inp, md=np.ascontiguousarray(inp["md"][:, ::-1]), ls=np.ascontiguousarray(inp["ls"][:, ::-1]), nvalid=np.ascontiguousarray(inp["nvalid"][:, ::-1]))


def with_duplicates(inp, b, side, pairs):
    """Exact duplicates: keypoint q of `side` becomes a copy of keypoint p (descriptor row and matchability) for every (p, q) in pairs."""
    md, ls = inp["md"].copy(), inp["ls"].copy()
    for p, q in pairs:
        md[b, side, q] = md[b, side, p]
        ls[b, side, q] = ls[b, side, p]
    return dict(inp, md=md, ls=ls)


# ------------------------------------------------------------------------------------------------ the launch rule, restated
def head_grid(B, npad):
    """(row blocks, column splits S) of launch_match_head_fused: the column tiles of a pair are split until the grid covers the chip."""
    nrb, ntile, S = npad // 128, npad // 64, 1
    while S < 8 and 2 * S <= ntile and nrb * B * S < 256:
        S *= 2
    return nrb, S


def renumbered(B, npad):
    nrb, S = head_grid(B, npad)
    return (nrb * S * B) % 8 == 0


def column_place(j, n1, S):
    """(column split, tile, 32-column half) that column j of a side with n1 valid columns is worked on in."""
    ntile = (n1 + 63) // 64
    t = j // 64
    sp = next(s for s in range(S) if ntile * s // S <= t < ntile * (s + 1) // S)
    return sp, t, (j % 64) // 32


def row_place(i):
    """(row block, row quarter) of row i."""
    return i // 128, (i % 128) // 32


# ------------------------------------------------------------------------------------------------ the operation
def split_hm16(x):
    """k_split_hm16 at scale 1: x = h + m + e, h and m fp16, round to nearest even (x f32; the residual x - h is exact in f32)."""
    x = np.asarray(x, np.float32)
    h = x.astype(np.float16)
    m = (x - h.astype(np.float32)).astype(np.float16)
    return h, m


def similarity(a, b, fmt, dtype):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if fmt == "f32":
        return a.astype(dtype) @ b.astype(dtype).T
    (ah, am), (bh, bm) = split_hm16(a), split_hm16(b)
    ah, am, bh, bm = (v.astype(dtype) for v in (ah, am, bh, bm))
    if dtype == np.float64:
        return ah @ (bh + bm).T + am @ bh.T      # (b_h + b_m is exact in fp64)
    return ah @ bh.T + ah @ bm.T + am @ bh.T


def top2(P, axis):
    """best, runner-up (multiplicity counted), arg-max (lowest index) along `axis` (1: of every row, 0: of every column)."""
    M = P if axis == 1 else P.T
    arg = M.argmax(1)
    best = M[np.arange(M.shape[0]), arg]
    if M.shape[1] < 2:
        return best, np.full_like(best, -np.inf), arg
    rest = M.copy()
    rest[np.arange(M.shape[0]), arg] = -np.inf
    return best, rest.max(1), arg


def evaluate(S, ls0, ls1, dtype):
    """The head's formula in `dtype`, in the association order of the reference expression."""
    S, ls0, ls1 = S.astype(dtype), np.asarray(ls0).astype(dtype), np.asarray(ls1).astype(dtype)
    rmax, cmax = S.max(1), S.max(0)
    rlog = np.log(np.exp(S - rmax[:, None]).sum(1, dtype=dtype))
    clog = np.log(np.exp(S - cmax[None, :]).sum(0, dtype=dtype))
    P = ((S - rmax[:, None]) - rlog[:, None]) + ((S - cmax[None, :]) - clog[None, :]) + (ls0[:, None] + ls1[None, :])
    best, second, m0 = top2(P, 1)
    colbest, col2, m1 = top2(P, 0)
    return dict(P=P, rlse=rmax + rlog, clse=cmax + clog, max0=best, max0b=second, m0=m0, colbest=colbest, col2=col2, m1=m1)


VALUES = ("rlse", "clse", "max0", "max0b", "colbest", "col2")      # what assertion 1 compares (rlse = rowmax + rowlog, clse = colmax + collog)


def filter_matches(max0, m0, m1, th):
    """[(i, m0[i])] for the rows with m1[m0[i]] == i and exp(max0[i]) > th, in row order."""
    return [(int(i), int(m0[i])) for i in range(len(m0)) if m1[m0[i]] == i and math.exp(float(max0[i])) > th]


def rule(best, second, colbest, col2, th, eps, dtype=np.float64, ulps=0):
    """The certificate's verdicts (a), (b), (c) of one pair -- True = that rule flags -- written with the comparisons of k_head_fused's last
    workgroup, in `dtype` arithmetic (float32: the kernel's own; `th` and `eps` are the floats the context holds).  ulps: log(th) moved by that
    many units in the last place (the device's logf and NumPy's may round differently)."""
    f = dtype
    best, second, colbest, col2 = (np.asarray(v).astype(f) for v in (best, second, colbest, col2))
    eps, th = f(eps), f(np.float32(th))
    with np.errstate(divide="ignore", invalid="ignore"):
        L = np.log(th) if th > 0 else f(-np.inf)
        for _ in range(abs(ulps)):
            L = np.nextafter(L, f(np.inf if ulps > 0 else -np.inf))
        a = bool(np.any((best >= L - eps) & ~(best - second > f(2.0) * eps)))
        b = bool(np.any((colbest >= L - eps) & ~(colbest - col2 > f(2.0) * eps)))
        c = bool(np.any(np.abs(best - L) <= eps))
    return a, b, c


def critical_eps(best, second, colbest, col2, th):
    """Every verdict of `rule` is a step in eps: (a) flags iff eps >= Ea = min_i max(L - best_i, gap_i / 2), (b) the same over the columns,
    (c) iff eps >= Ec = min_i |best_i - L|.  Returns (Ea, Eb, Ec) in fp64 -- the only values of eps at which the pair's verdicts change."""
    L = math.log(float(np.float32(th))) if th > 0 else -math.inf
    ea = float(np.min(np.maximum(L - best, (best - second) / 2.0)))
    eb = float(np.min(np.maximum(L - colbest, (colbest - col2) / 2.0)))
    ec = float(np.min(np.abs(best - L)))
    return ea, eb, ec


# ------------------------------------------------------------------------------------------------ a case's reference
class PairRef:
    def __init__(self, md, ls, n0, n1, fmt, keep_P=False):
        self.n0, self.n1, self.decides = int(n0), int(n1), n0 >= 2 and n1 >= 2      # kornia LightGlueMatcher._no_match
        if not self.decides:
            return
        a, b, l0, l1 = md[0, :n0], md[1, :n1], ls[0, :n0], ls[1, :n1]
        S = similarity(a, b, fmt, np.float64)
        self.r = evaluate(S, l0, l1, np.float64)
        r32 = evaluate(similarity(a, b, fmt, np.float32), l0, l1, np.float32)
        self.e32 = max(float(np.abs(r32[k].astype(np.float64) - self.r[k]).max()) for k in VALUES)
        # the split model against the unsplit fp64 product of the same descriptors: recorded, not asserted
        self.split_dist = float(np.abs(S - similarity(a, b, "f32", np.float64)).max()) if fmt != "f32" else 0.0
        self.row_gap, self.col_gap = self.r["max0"] - self.r["max0b"], self.r["colbest"] - self.r["col2"]
        self.P = self.r.pop("P") if keep_P else None
        if not keep_P:
            self.r.pop("P", None)

    def matches(self, th):
        return filter_matches(self.r["max0"], self.r["m0"], self.r["m1"], th) if self.decides else []

    def critical(self, th):
        return critical_eps(self.r["max0"], self.r["max0b"], self.r["colbest"], self.r["col2"], th)

    def verdicts(self, th, eps):
        return rule(self.r["max0"], self.r["max0b"], self.r["colbest"], self.r["col2"], th, eps) if self.decides else (False, False, False)


class CaseRef:
    def __init__(self, inp, fmt, keep_P=False):
        self.inp, self.fmt = inp, fmt
        self.pairs = [PairRef(inp["md"][b], inp["ls"][b], inp["nvalid"][b, 0], inp["nvalid"][b, 1], fmt, keep_P) for b in range(inp["B"])]
        dec = [p for p in self.pairs if p.decides]
        self.e32 = max(p.e32 for p in dec)
        self.budget = BUDGET_FACTOR * self.e32
        self.split_dist = max(p.split_dist for p in dec)
        self.rows, self.cols = sum(p.n0 for p in dec), sum(p.n1 for p in dec)

    def excluded(self, d):
        """(rows, columns) whose fp64 top-2 gap does not exceed 2 d: their arg-max is not compared."""
        dec = [p for p in self.pairs if p.decides]
        return sum(int((p.row_gap <= 2 * d).sum()) for p in dec), sum(int((p.col_gap <= 2 * d).sum()) for p in dec)


# ------------------------------------------------------------------------------------------------ the cases (ISSUE: the smallest sizes at which the partitioning changes)
RAGGED8 = [(63, 65), (129, 127), (1, 200), (200, 1), (5, 7), (256, 191), (2, 2), (97, 256)]      # tests/test_gpu_fused.py's list


def _varied64():
    rng = np.random.default_rng(64)
    nv = [(int(rng.integers(2, 513)), int(rng.integers(2, 513))) for _ in range(64)]
    nv[0], nv[17], nv[40], nv[63] = (512, 512), (512, 300), (129, 512), (512, 512)      # some full
    return nv


# id: (B, npad, [(n0, n1)] per pair, expected S, what it reaches)
CASES = {
    "np128": (1, 128, [(128, 128)], 2, "one row block, S = 2"),
    "np128_2x2": (1, 128, [(2, 2)], 2, "two keypoints per side"),
    "np256": (1, 256, [(130, 70)], 4, "second row block with 2 valid rows; 2 column tiles over S = 4 (empty splits)"),
    "np384": (1, 384, [(300, 384)], 4, "12 workgroups: no XCD renumbering"),
    "np512": (1, 512, [(512, 500)], 8, "S = 8"),
    "b8_np256": (8, 256, RAGGED8, 4, "no-match pairs inside a batch, S = 4"),
    "b64_np512": (64, 512, _varied64(), 1, "S = 1: rows finished by their own workgroup"),
    "np2176": (1, 2176, [(2100, 2176)], 8, "17 row blocks: second trip of the 16-partial column merge; S = 8; renumbering on"),
}
SEED = {k: 7100 + i for i, k in enumerate(CASES)}
TH = 0.1      # the threshold of the value / decision runs: best scores span -12 .. 0, so the list is a proper subset of the mutual pairs


def case_inputs(case, padding="garbage"):
    B, npad, nv, _, _ = CASES[case]
    return make_inputs(SEED[case], npad, nv, padding)


SAME_CASE = ("np128", "np128_2x2")      # the two runs of one case (B = 1, np = 128): d and e32 are the case's, taken over both runs


@functools.lru_cache(maxsize=None)
def case_ref(case, fmt):
    """The case's fp64 reference.  e32 (and the budget, 4 x e32) is the case's: over both runs for the two runs of SAME_CASE -- twelve numbers, which is all
    a 2 x 2 pair compares, measure no f32 evaluation's error (own_e32 keeps the run's own figure)."""
    ref = CaseRef(case_inputs(case), fmt)
    ref.own_e32 = ref.e32
    if case in SAME_CASE:
        ref.e32 = max([ref.e32] + [CaseRef(case_inputs(c), fmt).e32 for c in SAME_CASE if c != case])
        ref.budget = BUDGET_FACTOR * ref.e32
    return ref


# ------------------------------------------------------------------------------------------------ ties
TIE_CASES = ("np512", "np2176")
COL_KINDS = ("same half", "two halves of a tile", "different tiles", "different splits")
ROW_KINDS = ("same quarter", "different quarters", "different row blocks", "row blocks 0 and 16")


def col_kind(p, q, n1, S):
    (sp, tp, hp), (sq, tq, hq) = column_place(p, n1, S), column_place(q, n1, S)
    if sp != sq:
        return "different splits"
    if tp != tq:
        return "different tiles"
    return "same half" if hp == hq else "two halves of a tile"


def row_kind(p, q):
    (bp, qp), (bq, qq) = row_place(p), row_place(q)
    if bp != bq:
        return "row blocks 0 and 16" if {bp, bq} == {0, 16} else "different row blocks"
    return "same quarter" if qp == qq else "different quarters"


def _pick(owner_gap, owner_best, n, kind_of, kinds):
    """For every kind one (p, q), p < q: p is the arg-max of the owner (row or column) with the widest fp64 gap that still has a free partner q of
    that kind; q becomes a copy of p, so that owner's best is then tied between p and q."""
    used, out = set(), {}
    order = np.argsort(-owner_gap)
    for kind in kinds:
        for o in order:
            p = int(owner_best[o])
            if p in used:
                continue
            q = next((q for q in range(p + 1, n) if q not in used and kind_of(p, q) == kind), None)
            if q is not None:
                used.update((p, q)); out[kind] = (p, q)
                break
    return out


@functools.lru_cache(maxsize=None)
def tie_positions(case, fmt):
    """{"cols": {kind: (p, q)}, "rows": {kind: (p, q)}} for a tie case: the kinds its partitioning has (np512: one tile per column split and four row
    blocks, so "different tiles" within a split and "row blocks 0 and 16" exist at np2176 only)."""
    B, npad, nv, S, _ = CASES[case]
    n0, n1 = nv[0]
    r = case_ref(case, fmt).pairs[0]
    cols = _pick(r.row_gap, r.r["m0"], n1, lambda p, q: col_kind(p, q, n1, S), COL_KINDS)
    rows = _pick(r.col_gap, r.r["m1"], n0, row_kind, ROW_KINDS)
    return dict(cols=cols, rows=rows)


def tie_inputs(case, fmt, side):
    """The case with the duplicates of tie_positions copied in on `side` (1: tied columns, 0: tied rows)."""
    pos = tie_positions(case, fmt)["cols" if side == 1 else "rows"]
    return with_duplicates(case_inputs(case), 0, side, sorted(pos.values()))


@functools.lru_cache(maxsize=None)
def tie_ref(case, fmt, side):
    return CaseRef(tie_inputs(case, fmt, side), fmt, keep_P=True)


def tied_entries(ref_pair, groups, side, d):
    """[(index, p)]: the rows (side 1: tied columns) or columns (side 0: tied rows) whose fp64 best lies in a duplicated group {p, q}, p < q, with more
    than 2 d to the largest value outside the group.  There the arg-max must be p and the runner-up must equal the best.  (The two copies agree in fp64
    to the rounding of the matrix product, which a BLAS may order differently for two columns: 1e-9 stands for "equal".)"""
    P = ref_pair.P if side == 1 else ref_pair.P.T
    out = []
    for p, q in groups:
        tied = np.abs(P[:, p] - P[:, q]) <= 1.0e-9
        rest = P.copy()
        rest[:, [p, q]] = -np.inf
        outside = rest.max(1)
        for o in np.nonzero(tied & (np.minimum(P[:, p], P[:, q]) - outside > 2.0 * d))[0]:
            out.append((int(o), p))
    return out


# ------------------------------------------------------------------------------------------------ the eps / threshold table of the flag tests
FLAG_CASE = "b8_np256"
MARGIN = 8.0      # every eps lies at least 8 x (the value budget) from the values at which an fp64 verdict changes


@functools.lru_cache(maxsize=None)
def eps_table(fmt):
    """([dict(kind, th, eps, swap, pair, expect)], margin) on FLAG_CASE, from fp64 alone.  `expect`: per pair the (a, b, c) the fp64 rule gives for the inputs
    the entry runs on; `pair`: the pair the entry was built on (None: all of them) -- there its eps keeps `margin` = MARGIN x the case's value budget from
    every critical value (pair_margin), so neither the kernel's rounding of the scores nor that of logf(th) can decide a comparison."""
    ref = case_ref(FLAG_CASE, fmt)
    dec = [b for b, p in enumerate(ref.pairs) if p.decides]
    crit0 = {b: ref.pairs[b].critical(0.0) for b in dec}
    table = []

    def entry(kind, th, eps, pair, swap=False):
        th, eps = float(np.float32(th)), float(np.float32(eps))
        exp = [p.verdicts(th, eps) for p in ref.pairs]
        if swap:      # the transposed pair: (a) and (b) change places (swapped entries use th = 0, where (c) never flags below eps = inf)
            exp = [(b_, a_, c_) for a_, b_, c_ in exp]
        table.append(dict(kind=kind, th=th, eps=eps, swap=swap, pair=pair, expect=exp))

    # nothing flags in any pair: half the smallest critical value of the batch
    entry("none", 0.0, min(min(crit0[b][:2]) for b in dec) / 2.0, None)
    # only (a): smallest row half-gap < eps < smallest column half-gap, on the pair where the two are furthest apart; only (b): that pair transposed
    b = max(dec, key=lambda b: crit0[b][1] - crit0[b][0])
    entry("only a", 0.0, (crit0[b][0] + crit0[b][1]) / 2.0, b)
    entry("only b", 0.0, (crit0[b][0] + crit0[b][1]) / 2.0, b, swap=True)
    # only (c): th = exp(best_i) of a row with a wide gap -- of all pairs' 16 widest rows the one that leaves most room under the two gap rules
    room, pick = -1.0, None
    for b in dec:
        p = ref.pairs[b]
        for i in np.argsort(-p.row_gap)[:16]:
            th = float(np.float32(math.exp(p.r["max0"][i])))
            ea, eb, _ = p.critical(th)
            if min(ea, eb) > room:
                room, pick = min(ea, eb), (b, th)
    entry("only c", pick[1], room / 2.0, pick[0])
    # a batch in which some pairs flag and some do not: the middle of the widest interval free of critical values that separates two pairs
    lo, hi = min(min(crit0[b][:2]) for b in dec), max(min(crit0[b][:2]) for b in dec)
    allc = sorted(c for b in dec for c in crit0[b][:2] if lo <= c <= hi)
    k = max(range(len(allc) - 1), key=lambda k: allc[k + 1] - allc[k])
    entry("mixed", 0.0, (allc[k] + allc[k + 1]) / 2.0, None)
    entry("all", 0.0, math.inf, None)
    entry("eps 0", 0.0, 0.0, None)
    return table, MARGIN * ref.budget


def pair_margin(ref, e, b):
    """The distance of the entry's eps from the nearest critical value of pair b (fp64); inf where nothing can change (eps = inf, a pair without a decision)."""
    if not ref.pairs[b].decides or not math.isfinite(e["eps"]):
        return math.inf
    return min(abs(e["eps"] - c) for c in ref.pairs[b].critical(e["th"]) if math.isfinite(c))
