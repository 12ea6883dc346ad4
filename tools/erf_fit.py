#!/usr/bin/env python3
"""Coefficients of the two-product block tail's erf (csrc/gn_ffn128.hip, `if constexpr (PROD == 2)`).

The level-2 GELU of k_ffn128 evaluates, per hidden value y (after LayerNorm),

    a  = min(|y|, C)
    m  = a * P(a)                      P = c0 + c1 a + c2 a^2 + c3 a^3 (... degree D), Horner in f32 fma
    u  = 1 - exp2(-m)                  ~ erf(|y| / sqrt 2)
    hy = 0.5 y
    out = fma(|hy|, u, hy)             = 0.5 y (1 + erf(y / sqrt 2))

so P approximates g(a) = -log2(erfc(a / sqrt 2)) / a: the 1 / sqrt 2 of the erf argument is folded into the coefficients and the clamp point.
This script fits P in the minimax sense on [0, C], the error of P weighted by the sensitivity of u to it (du/dP = ln 2 * a * 2^(-a g)), so
that what is levelled is the absolute error of the erf -- the GELU's error is 0.5 |y| times that.  Lawson's iteratively reweighted least
squares on a dense Chebyshev-spaced grid (numpy only); the result is rounded to f32 and THEN measured: the f32 operation sequence above,
against fp64, over a dense grid and over every fp16 value in [-12, 12].

    python tools/erf_fit.py [--degree D] [--clamp 5.75]

prints the report that DESIGN.md 10.2 quotes and the literals for the kernel (tests/test_erf_level2_host.py parses them out of the kernel
source and repeats the measurement).  Without --degree it takes the lowest degree whose error is below the bound with 4x margin: 3.  The
kernel carries `--degree 4`: on the GPU degree 3 moved the level's calibrated eps by more than its scatter over calibration samples
(profiles/erf_level2_certificate.json), which this script cannot see.
"""
from __future__ import annotations

import argparse
import math

import numpy as np

BOUND = 2.0 ** -13          # |gelu error| <= BOUND * |y|: half the fp16 rounding step the level applies to the same value


def erfc64(x: np.ndarray) -> np.ndarray:
    return np.array([math.erfc(float(v)) for v in np.ravel(x)], dtype=np.float64).reshape(np.shape(x))


def erf64(x: np.ndarray) -> np.ndarray:
    return np.array([math.erf(float(v)) for v in np.ravel(x)], dtype=np.float64).reshape(np.shape(x))


def g_exact(a: np.ndarray) -> np.ndarray:
    """-log2(erfc(a / sqrt 2)) / a, with its limit sqrt(2 / pi) / ln 2 at 0."""
    a = np.asarray(a, dtype=np.float64)
    out = np.full(a.shape, math.sqrt(2.0 / math.pi) / math.log(2.0))
    nz = a > 1e-9
    out[nz] = -np.log2(erfc64(a[nz] / math.sqrt(2.0))) / a[nz]
    return out


def fit(degree: int, clamp: float, n: int = 4001, iters: int = 400) -> np.ndarray:
    """Weighted minimax coefficients c0..cD (fp64) of P on [0, clamp]."""
    a = 0.5 * clamp * (1.0 - np.cos(np.pi * (np.arange(n) + 0.5) / n))        # Chebyshev-spaced: dense at both ends
    g = g_exact(a)
    sens = math.log(2.0) * a * np.exp2(-a * g)                                # d(1 - 2^(-a P)) / dP at P = g
    V = np.vander(a, degree + 1, increasing=True)
    lw = np.full(n, 1.0 / n)                                                  # Lawson weights
    c = None
    for _ in range(iters):
        w = np.sqrt(lw) * sens
        c, *_ = np.linalg.lstsq(V * w[:, None], g * w, rcond=None)
        err = np.abs(sens * (V @ c - g))
        lw = lw * err
        lw = lw / lw.sum()
    return c


def f32_fma(x, y, z):
    """One f32 fused multiply-add: the product of two f32 is exact in fp64."""
    return (np.asarray(x, np.float32).astype(np.float64) * np.asarray(y, np.float32).astype(np.float64)
            + np.asarray(z, np.float32).astype(np.float64)).astype(np.float32)


def gelu_level2(y, coef, clamp):
    """The kernel's operation sequence in f32 (coef: c0..cD as f32, clamp as f32).  Returns (gelu, u)."""
    y = np.asarray(y, np.float32)
    a = np.minimum(np.abs(y), np.float32(clamp))
    p = f32_fma(np.float32(coef[-1]), a, np.float32(coef[-2]))
    for k in range(len(coef) - 3, -1, -1):
        p = f32_fma(p, a, np.float32(coef[k]))
    m = (p * a).astype(np.float32)
    e = np.exp2(-m).astype(np.float32)
    u = (np.float32(1.0) - e).astype(np.float32)
    hy = (np.float32(0.5) * y).astype(np.float32)
    return f32_fma(np.abs(hy), u, hy), u


def gelu64(y):
    y = np.asarray(y, np.float64)
    return 0.5 * y * (1.0 + erf64(y / math.sqrt(2.0)))


def fp16_values(lim: float) -> np.ndarray:
    v = np.arange(1 << 16, dtype=np.uint16).view(np.float16).astype(np.float32)
    return v[np.isfinite(v) & (np.abs(v) <= lim)]


def report(coef32, clamp32) -> dict:
    dense = np.linspace(-12.0, 12.0, 2_400_001).astype(np.float32)
    h16 = fp16_values(12.0)
    out = {}
    for name, y in (("dense grid, 2.4e6 points in [-12, 12]", dense), ("every fp16 value in [-12, 12]", h16)):
        ge, u = gelu_level2(y, coef32, clamp32)
        y64 = y.astype(np.float64)
        erf_err = np.abs(np.copysign(u.astype(np.float64), y64) - erf64(y64 / math.sqrt(2.0)))
        d = np.abs(ge.astype(np.float64) - gelu64(y64))
        nz = y64 != 0
        out[name] = {"n": int(y.size), "max_abs_erf_err": float(erf_err.max()), "max_abs_gelu_err": float(d.max()),
                     "max_gelu_err_over_abs_y": float((d[nz] / np.abs(y64[nz])).max()), "bound_over_worst": float(BOUND / (d[nz] / np.abs(y64[nz])).max())}
    a = np.linspace(0.0, float(clamp32), 200001).astype(np.float32)
    p = f32_fma(np.float32(coef32[-1]), a, np.float32(coef32[-2]))
    for k in range(len(coef32) - 3, -1, -1):
        p = f32_fma(p, a, np.float32(coef32[k]))
    m = (p * a).astype(np.float32)
    out["exponent m = a P(a)"] = {"monotone_on_clamp_range": bool(np.all(np.diff(m.astype(np.float64)) >= 0)), "m_at_clamp": float(m[-1]),
                                 "u_at_clamp_is_one": bool(np.float32(1.0) - np.exp2(-m[-1]).astype(np.float32) == np.float32(1.0))}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--degree", type=int, default=0, help="0 = the lowest degree that meets the bound with 4x margin")
    ap.add_argument("--clamp", type=float, default=5.75, help="clamp point C in |y| (u(C) must be exactly 1 in f32: m(C) > 25)")
    args = ap.parse_args()
    for degree in ([args.degree] if args.degree else [2, 3, 4, 5]):
        c = fit(degree, args.clamp)
        c32 = c.astype(np.float32)
        clamp32 = np.float32(args.clamp)
        rep = report(c32, clamp32)
        worst = max(v["max_gelu_err_over_abs_y"] for k, v in rep.items() if "max_gelu_err_over_abs_y" in v)
        ok = worst * 4.0 <= BOUND and rep["exponent m = a P(a)"]["monotone_on_clamp_range"] and rep["exponent m = a P(a)"]["u_at_clamp_is_one"]
        print(f"degree {degree}, clamp |y| <= {float(clamp32)!r}: bound 2^-13 |y| = {BOUND:.4e} |y|, worst {worst:.4e} |y| (margin {BOUND / worst:.1f}x) -> {'TAKEN' if ok else 'rejected'}")
        for k, v in rep.items():
            print(f"  {k}: " + ", ".join(f"{kk} = {vv:.4e}" if isinstance(vv, float) else f"{kk} = {vv}" for kk, vv in v.items()))
        if ok or args.degree:
            print("  literals for csrc/gn_ffn128.hip (c0 .. cD, then the clamp):")
            print("  constexpr float kErf2C[%d] = {%s};" % (degree + 1, ", ".join(f"{float(x)!r}f" for x in c32)))
            print(f"  constexpr float kErf2Clamp = {float(clamp32)!r}f;")
            break


if __name__ == "__main__":
    main()
