"""numpy restatement of the size-3 Fisher-z test of the table kernel (csrc/fw_fz_core.h, fz_seg_body): the conservative Float32 screen
of the fast loop (the `#if FW_FZ_SCREEN` block) next to the exact sequence (pc_l1 / pc_l2 / pc_l3) it stands in front of, both from the same
ten matrix entries.  Helper module: no tests in it.

It CHOOSES INPUTS AND COUNTS COVERAGE; it is never an expected value.  Expected values come from the oracle (oracle/fw_oracle.c);
tests/test_screen_model_cpu.py anchors the exact half on the oracle to the bit before it relies on either half.

One size-3 test conditions X, Y on (z1, zj, zk) = accepted[(i, j, k)], i < j < k, peeled in that order (statfuns.jl:44-53).  Operands
(all Float32 matrix entries), as keyword arrays of one shape:

    cXY                      cor[X][Y]
    cXz, cYz                 cor[X][z1], cor[Y][z1]
    cXj, cYj, cjz            cor[X][zj], cor[Y][zj], cor[zj][z1]
    cXk, cYk, ckz            cor[X][zk], cor[Y][zk], cor[zk][z1]
    cjk                      cor[zk][zj]

Arithmetic notes.  Every Float32 operation is a numpy float32 operation (IEEE, round to nearest even: the device's).  fmaf is the exact
product and sum rounded once (fma32 below).  v_rcp_f32 is documented to 1 ulp: the screen is evaluated with the correctly rounded
reciprocal and with its two neighbours (rcp_ulp = 0, -1, +1).  round(x, digits = 5) is rint(x * 1e5) / 1e5 in the value's own type (the
device's three-instruction division by 1e5 is the correctly rounded quotient: tests/test_oracle_golden.py).
"""
import itertools

import numpy as np

f32 = np.float32
f64 = np.float64

# the kernel's constants (fw_fz_core.h, "cheap screen")
DL_C1 = 4.8e-5      # dl = DL_C1 / d1 + DL_C2
DL_C2 = 7.4e-5
T_FACTOR = 1.0002   # on the bound the screen compares with
PUB_FACTOR = 1.00001  # on the bound the exact path publishes
G_D1 = 0.01         # guards: d1 > G_D1, g > G_G, Pb > dl, Pc > dl, Nlo > 0
G_G = 0.02

OPERANDS = ("cXY", "cXz", "cYz", "cXj", "cYj", "cjz", "cXk", "cYk", "ckz", "cjk")


def _f(x):
    return np.asarray(x, dtype=f32)


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays: a * b is exact in float64 (48 bits), the sum is rounded to 53 bits and then to 24 -- wrong only where
    the 53-bit sum sits exactly on a float32 tie that the exact sum is not on; those (rare) elements are redone with the sum rounded to
    odd, which makes the second rounding the correct single one."""
    a, b, c = np.broadcast_arrays(_f(a), _f(b), _f(c))
    p = a.astype(f64) * b.astype(f64)
    c64 = c.astype(f64)
    s = p + c64
    bits = np.ascontiguousarray(s).view(np.int64)
    tie = (bits & 0x1FFFFFFF) == 0x10000000
    if tie.any():
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)  # TwoSum: s + err = p + c exactly
        fix = tie & (err != 0.0) & np.isfinite(s)
        if fix.any():
            s = s.copy()
            s[fix] = np.nextafter(s[fix], np.where(err[fix] > 0.0, np.inf, -np.inf))  # (a tie pattern is even: one step makes it odd)
    return s.astype(f32)


def round5_32(x):
    x = _f(x)
    with np.errstate(invalid="ignore"):
        y = np.rint(x * f32(100000.0)) / f32(100000.0)
    return np.where(np.isfinite(y), y, x).astype(f32)


def round5_64(x):
    x = np.asarray(x, f64)
    with np.errstate(invalid="ignore"):
        y = np.rint(x * 100000.0) / 100000.0
    return np.where(np.isfinite(y), y, x)


def _clamp(v, is32):
    """v < -1 -> -1.0, v >= 1 -> 1.0 (Float64 literals: the value stops being a Float32 value); a NaN stays."""
    lo, hi = v < -1.0, v >= 1.0
    v = np.where(lo, -1.0, np.where(hi, 1.0, v))
    return v, is32 & ~lo & ~hi


def level1(xy, xz, yz):
    """pc_l1 (statfuns.jl:32-41, ContType = Float32) -> (value as float64, still-a-Float32-value flag, e, d)."""
    xy, xz, yz = _f(xy), _f(xz), _f(yz)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = round5_32(xy - xz * yz)
        d = np.sqrt(f32(1.0) - xz * xz) * np.sqrt(f32(1.0) - yz * yz)
        nz = ~(d == f32(0.0))  # (a NaN denominator divides: NaN)
        v = np.where(nz, (e / np.where(nz, d, f32(1.0))).astype(f64), 0.0)
    v, is32 = _clamp(v, nz)
    return v, is32, e, d


def level2(a, a32, b, b32, c, c32):
    """pc_l2 (statfuns.jl:44-62) on level-1 children: Float32 arithmetic for `a - b c` and the root of 1 - b^2 where the children are still
    Float32 values, Float64 where a literal 0 / +-1 replaced one; the root of 1 - c^2 always in Float64 (statfuns.jl:52, `^2.0`)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        bf, cf, af = b.astype(f32), c.astype(f32), a.astype(f32)
        p32 = b32 & c32
        prod = np.where(p32, (bf * cf).astype(f64), b * c)
        ev = np.where(a32 & p32, round5_32(af - prod.astype(f32)).astype(f64), round5_64(a - prod))
        d1 = np.where(b32, np.sqrt(f32(1.0) - bf * bf).astype(f64), np.sqrt(1.0 - b * b))
        d2 = np.sqrt(1.0 - c * c)
        den = d1 * d2
        z = den == 0.0
        v = np.where(z, 0.0, ev / np.where(z, 1.0, den))
    v, _ = _clamp(v, np.ones(v.shape, bool))
    return v


def level3_parts(a, b, c):
    """pc_l3 (all-Float64 children), first half: ev = round5(a - b c), xb = 1 - b^2, xc = 1 - c^2."""
    with np.errstate(invalid="ignore"):
        return round5_64(a - b * c), 1.0 - b * b, 1.0 - c * c


def level3_finish(ev, xb, xc):
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.sqrt(xb) * np.sqrt(xc)
        z = den == 0.0
        v = np.where(z, 0.0, ev / np.where(z, 1.0, den))
    v, _ = _clamp(v, np.ones(v.shape, bool))
    return v


def exact(**c):
    """The exact sequence of one size-3 test -> dict: stat = rho(X, Y | z1, zj, zk) (what the oracle returns), its halves ev, xb, xc
    (|stat|^2 = ev^2 / (xb xc) where no clamp acts), the table entries the screen reads (LXj, LYj, LXk, LYk, A2j, Float32 roots) and
    `clean` / `f1ok`: the conditions under which the fast loop commits the test (no NaN, no Float64 literal among the table entries /
    in rho(zk, zj | z1)); the screen itself only looks at `clean`."""
    c = {k: _f(c[k]) for k in OPERANDS}
    A1, A1f, _, _ = level1(c["cXY"], c["cXz"], c["cYz"])
    LXj, LXjf, _, _ = level1(c["cXj"], c["cXz"], c["cjz"])
    LYj, LYjf, _, _ = level1(c["cYj"], c["cYz"], c["cjz"])
    LXk, LXkf, _, _ = level1(c["cXk"], c["cXz"], c["ckz"])
    LYk, LYkf, _, _ = level1(c["cYk"], c["cYz"], c["ckz"])
    F1, F1f, e1, d1 = level1(c["cjk"], c["ckz"], c["cjz"])
    A2j = level2(A1, A1f, LXj, LXjf, LYj, LYjf)
    A2k = level2(A1, A1f, LXk, LXkf, LYk, LYkf)  # (the zk entry's own rho(X, Y | z1, zk): part of its clean flag)
    D2 = level2(LXk, LXkf, LXj, LXjf, F1, F1f)
    E2 = level2(LYk, LYkf, LYj, LYjf, F1, F1f)
    ev, xb, xc = level3_parts(A2j, D2, E2)
    stat = level3_finish(ev, xb, xc)
    nn = lambda *v: np.logical_and.reduce([x == x for x in v])
    clean = LXjf & LYjf & LXkf & LYkf & nn(LXj, LYj, LXk, LYk, A2j, A2k)  # the two table entries (bits 28-30 of their flag words)
    f1ok = F1f & nn(F1)                                                   # ... and rho(zk, zj | z1) still a Float32 value
    with np.errstate(invalid="ignore"):
        fx, fy = LXj.astype(f32), LYj.astype(f32)
        rjx, rjy = np.sqrt(f32(1.0) - fx * fx), np.sqrt(f32(1.0) - fy * fy)
        rj1, rk1 = np.sqrt(f32(1.0) - c["cjz"] * c["cjz"]), np.sqrt(f32(1.0) - c["ckz"] * c["ckz"])
    return dict(stat=stat, ev=ev, xb=xb, xc=xc, A2j=A2j, D2=D2, E2=E2, F1=F1, e1=e1, d1=d1, clean=clean, f1ok=f1ok,
                LXj=fx, LYj=fy, LXk=LXk.astype(f32), LYk=LYk.astype(f32), rjx=rjx, rjy=rjy, rj1=rj1, rk1=rk1,
                cjz=c["cjz"], ckz=c["ckz"], cjk=c["cjk"])


def rcp32(d, ulp=0):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (f32(1.0) / _f(d)).astype(f32)
    if ulp > 0:
        r = np.nextafter(r, f32(np.inf))
    elif ulp < 0:
        r = np.nextafter(r, f32(-np.inf))
    return r


def screen(ex, rcp_ulp=0, c1=DL_C1, c2=DL_C2, scale=1.0):
    """The screen of the fast loop on the table entries of exact(): every intermediate, the guards, and both sides of its comparison.
    dl = fmaf(scale c1, rcp(d1), scale c2).  -> dict with
      guards  every guard holds (clean entries, d1 > 0.01, g > 0.02, Pb > dl, Pc > dl, Nlo > 0);
      nl2, den  Float32 Nlo^2 and (Pb + dl)(Pc + dl): the test is skipped against a bound T when nl2 > T den in Float32;
      LB      nl2 / den in Float64: the screen's lower bound of |stat|^2."""
    k1, k2 = f32(scale * c1), f32(scale * c2)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        e1s = ex["cjk"] - ex["ckz"] * ex["cjz"]
        d1s = ex["rk1"] * ex["rj1"]
        inv1 = rcp32(d1s, rcp_ulp)
        Fs = e1s * inv1
        dl = fma32(k1, inv1, k2)
        gs = fma32(-Fs, Fs, f32(1.0))
        nD = fma32(-ex["LXj"], Fs, ex["LXk"])
        nE = fma32(-ex["LYj"], Fs, ex["LYk"])
        rg = ex["rjx"] * gs
        Pb = fma32(-nD, nD, ex["rjx"] * rg)
        Pc = fma32(-nE, nE, ex["rjy"] * ex["rjy"] * gs)
        Nm = fma32(-nD, nE, ex["A2j"].astype(f32) * rg * ex["rjy"])
        Nlo = np.abs(Nm) - dl
        guards = ex["clean"] & (d1s > f32(G_D1)) & (gs > f32(G_G)) & (Pb > dl) & (Pc > dl) & (Nlo > f32(0.0))
        nl2 = Nlo * Nlo
        den = (Pb + dl) * (Pc + dl)
        LB = nl2.astype(f64) / den.astype(f64)
    return dict(guards=guards, d1=d1s, inv1=inv1, F=Fs, dl=dl, g=gs, nD=nD, nE=nE, Pb=Pb, Pc=Pc, Nm=Nm, Nlo=Nlo, nl2=nl2, den=den, LB=LB)


def violations(ex, sc, factor=T_FACTOR):
    """Tests the screen may skip although the exact value does not clear the bound it was screened against: with T the largest bound
    the test is still skipped against, T den <= nl2 (1 + 2^-23) in Float32, and the bookkeeping needed the value when
    ev^2 <= (T / factor) xb xc (the validation build's rule, -DFW_FZ_FASTDBG=5) -- so: guards and not ev^2 > LB (1 + 2^-23) / factor * xb xc.
    A NaN on the exact side, or a clamped rho(zk, zj | z1), counts as a violation."""
    with np.errstate(invalid="ignore", over="ignore"):
        ok = ex["ev"] * ex["ev"] > (sc["LB"] * (1.0 + 2.0 ** -23) / factor) * (ex["xb"] * ex["xc"])
    return sc["guards"] & ~(ok & ex["f1ok"])


def ratio(ex, sc):
    """exact |stat|^2 / LB where the guards hold (inf elsewhere): a violation needs a ratio <= 1 / 1.0002."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = ex["ev"] * ex["ev"] / (ex["xb"] * ex["xc"])
        r = q / sc["LB"]
    return np.where(sc["guards"], r, np.inf)


def published(ex):
    """The bound the exact path publishes for a test it takes as lane best: |stat|^2 rounded up into Float32."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        e2 = (ex["ev"] * ex["ev"]).astype(f32)
        return (e2 / (ex["xb"].astype(f32) * ex["xc"].astype(f32))) * f32(PUB_FACTOR)


# ---- matrices ----------------------------------------------------------------------------------------------------------------------

def tuple_matrix(**c):
    """5 x 5 Float32 matrix over [X, Y, z1, zj, zk] = [0..4] holding one operand tuple (scalars)."""
    m = np.eye(5, dtype=f32)
    for (u, v), k in {(0, 1): "cXY", (0, 2): "cXz", (1, 2): "cYz", (0, 3): "cXj", (1, 3): "cYj", (3, 2): "cjz", (0, 4): "cXk",
                      (1, 4): "cYk", (4, 2): "ckz", (4, 3): "cjk"}.items():
        m[u, v] = m[v, u] = f32(c[k])
    return m


def job_operands(cm, X, Y, acc):
    """Operand arrays of ALL size-3 tests of the job (X, Y, accepted), in the enumeration's order (lexicographic positions i < j < k;
    rank r of the job is element r: size 3 comes first) -> (dict of operands, (i, j, k) position arrays)."""
    cm = np.asarray(cm, f32)
    a = len(acc)
    pos = np.array(list(itertools.combinations(range(a), 3)), dtype=np.int64).reshape(-1, 3)
    z = np.asarray(acc, np.int64)
    z1, zj, zk = z[pos[:, 0]], z[pos[:, 1]], z[pos[:, 2]]
    c = dict(cXY=np.full(len(pos), cm[X, Y], f32), cXz=cm[X, z1], cYz=cm[Y, z1], cXj=cm[X, zj], cYj=cm[Y, zj], cjz=cm[zj, z1],
             cXk=cm[X, zk], cYk=cm[Y, zk], ckz=cm[zk, z1], cjk=cm[zk, zj])
    return c, pos


def job_model(cm, X, Y, acc, **kw):
    c, pos = job_operands(cm, X, Y, acc)
    ex = exact(**c)
    return ex, screen(ex, **kw), pos


def cor_from_loadings(W, psi):
    """Float32 correlation matrix of the factor model  v = W f + sqrt(psi) e  (f, e independent standard normal), computed in Float64:
    symmetric, unit diagonal, |entry| <= 1."""
    W = np.asarray(W, f64)
    S = W @ W.T + np.diag(np.asarray(psi, f64))
    d = 1.0 / np.sqrt(np.diag(S))
    cm = (S * d[:, None] * d[None, :]).astype(f32)
    cm = np.minimum(cm, cm.T)
    np.fill_diagonal(cm, 1.0)
    return np.clip(cm, -1.0, 1.0)


# ---- operand generators --------------------------------------------------------------------------------------------------------
def draw_tuples(rng, n, window):
    """n operand tuples drawn into one guard window.  The level-1 values given z1 (F = rho(zk, zj | z1), LXj, ...) are chosen first and
    the matrix entries backed out of them (cor[v][w] = c_v c_w + r_v r_w rho), so the window is hit on purpose:
      d1   d1 = r_j r_k in [0.009, 0.02]  (both sides of the guard at 0.01; round5's 5e-6 on e1 becomes up to 5.6e-4 on F)
      g    g = 1 - F^2 in [0.015, 0.04]   (both sides of 0.02), d1 in [0.02, 1]
      P    Pb or Pc within [0, 4 dl]      (both sides of dl; D2 / E2 next to +-1, where the exact path clamps)
      N    |Num| within [0, 4 dl]         (both sides of Nlo = 0)"""
    U = lambda lo, hi: rng.uniform(lo, hi, n)
    sgn = lambda: rng.choice([-1.0, 1.0], n)
    if window == "d1":
        d1 = U(0.009, 0.02)
        rj = np.sqrt(d1) * np.exp(U(-0.7, 0.7))
        rk = d1 / rj
    else:
        lo = 0.02 if window == "g" else 0.012
        d1 = np.exp(U(np.log(lo), 0.0))
        rj = np.sqrt(d1) * np.exp(U(-0.5, 0.5) * np.minimum(1.0, -np.log(d1)))
        rj = np.minimum(rj, 1.0)
        rk = np.minimum(d1 / rj, 1.0)
    cjz, ckz = sgn() * np.sqrt(1.0 - rj * rj), sgn() * np.sqrt(1.0 - rk * rk)
    cXz, cYz = U(-0.8, 0.8), U(-0.8, 0.8)
    rX, rY = np.sqrt(1.0 - cXz ** 2), np.sqrt(1.0 - cYz ** 2)
    F = sgn() * np.sqrt(1.0 - U(0.015, 0.04)) if window == "g" else U(-0.97, 0.97)
    g = 1.0 - F * F
    LXj, LYj = U(-0.9, 0.9), U(-0.9, 0.9)
    dl = 4.8e-5 / (rj * rk) + 7.4e-5
    if window == "P":
        # Pb = (1 - LXj^2) g - nD^2 with nD = LXk - LXj F: choose Pb, solve for LXk (and the same for Pc / LYk on half of the tuples)
        both = rng.random(n) < 0.5
        tb, tc = U(0.0, 4.0) * dl, U(0.0, 4.0) * dl
        LXk = LXj * F + sgn() * np.sqrt(np.maximum((1.0 - LXj ** 2) * g - tb, 0.0))
        LYk_p = LYj * F + sgn() * np.sqrt(np.maximum((1.0 - LYj ** 2) * g - tc, 0.0))
        LYk = np.where(both, LYk_p, U(-0.9, 0.9))
        LXk, LYk = np.clip(LXk, -0.999, 0.999), np.clip(LYk, -0.999, 0.999)
    else:
        LXk, LYk = U(-0.9, 0.9), U(-0.9, 0.9)
    if window == "N":
        # Num = (A1 - LXj LYj) g - nD nE: choose Num, solve for A1 = rho(X, Y | z1)
        nD, nE = LXk - LXj * F, LYk - LYj * F
        A1 = LXj * LYj + (sgn() * U(0.0, 4.0) * dl + nD * nE) / g
        A1 = np.clip(A1, -0.999, 0.999)
    else:
        A1 = U(-0.95, 0.95)
    c = dict(cXY=A1 * rX * rY + cXz * cYz, cXz=cXz, cYz=cYz, cXj=LXj * rX * rj + cXz * cjz, cYj=LYj * rY * rj + cYz * cjz, cjz=cjz,
             cXk=LXk * rX * rk + cXz * ckz, cYk=LYk * rY * rk + cYz * ckz, ckz=ckz, cjk=F * rj * rk + cjz * ckz)
    return {k: np.clip(v, -1.0, 1.0).astype(f32) for k, v in c.items()}


def in_window(sc, window):
    dl = sc["dl"].astype(f64)
    if window == "d1":
        return sc["d1"] < f32(0.02)
    if window == "g":
        return sc["g"] < f32(0.04)
    if window == "P":
        return (sc["Pb"] < 3.0 * dl) | (sc["Pc"] < 3.0 * dl)
    return sc["Nlo"] < 2.0 * dl


WINDOWS = ("d1", "g", "P", "N")


# ---- directed search -------------------------------------------------------------------------------------------------------------
ULPS = (0, -1, 1)


def scale_estimate(c):
    """Per tuple, an estimate of the largest scale s of dl at which the tuple is a violation (0: at none), from ONE evaluation of the screen:
    its intermediates do not depend on dl, so LB(s) = (|Num| - s dl)^2 / ((Pb + s dl)(Pc + s dl)) is bisected in Float64 against
    1.0002 |stat|^2 under the guards Pb, Pc, |Num| > s dl.  The objective of directed_search; critical_scale() is the measurement."""
    ex = exact(**c)
    out = np.zeros(len(c["cXY"]))
    with np.errstate(all="ignore"):
        q = ex["ev"] ** 2 / (ex["xb"] * ex["xc"])
        tgt = np.where(ex["f1ok"] & np.isfinite(q), q * T_FACTOR, 0.0)
        for u in ULPS:
            sc = screen(ex, rcp_ulp=u)
            N, Pb, Pc, dl = (np.abs(sc["Nm"]).astype(f64), sc["Pb"].astype(f64), sc["Pc"].astype(f64), sc["dl"].astype(f64))
            base = ex["clean"] & (sc["d1"] > f32(G_D1)) & (sc["g"] > f32(G_G)) & (Pb > 0) & (Pc > 0) & (N > 0)
            top = np.minimum(np.minimum(np.minimum(Pb, Pc), N) / dl * 0.999999, 1.5)
            LB = lambda s: (N - s * dl) ** 2 / ((Pb + s * dl) * (Pc + s * dl))
            lo, hi = np.zeros_like(q), top
            at_top = LB(top) >= tgt
            for _ in range(16):
                mid = 0.5 * (lo + hi)
                v = LB(mid) >= tgt
                lo, hi = np.where(v, mid, lo), np.where(v, hi, mid)
            s = np.where(base & (LB(0.0) >= tgt), np.where(at_top, top, lo), 0.0)
            out = np.maximum(out, np.nan_to_num(s))
    return out


def _grid_candidates(x, rng, shape):
    """Float32 candidates next to x: a few ulps either side, and steps of about 1e-6, 5e-6 and 1e-5 (round5's grid, its half and its
    tenth) -- the moves that walk e1, nD, nE and ev across and onto the half-points of round5."""
    k = rng.integers(-3, 4, shape).astype(f64)
    kind = rng.integers(0, 4, shape)
    step = np.where(kind == 0, 6e-8, np.where(kind == 1, 1e-6, np.where(kind == 2, 5e-6, 1e-5)))
    return np.clip(x[..., None].astype(f64) + k * step * (0.5 + rng.random(shape)), -1.0, 1.0).astype(f32)


def directed_search(seed=7, pop=3000, sweeps=4, cand=20):
    """Coordinate descent, a whole population at once: every free matrix entry of every tuple in turn (cjk moves e1; cXk, cYk move nD, nE;
    cXY moves ev; cXj, cYj all of them) tries `cand` neighbours and keeps the one that raises scale_estimate -- i.e. lines the round5
    errors of e1, nD, nE and ev up with the signs that shrink the exact |stat|^2 against the screen's lower bound.  Starts: tuples of the
    near-collinear and the Pb / Pc windows, half of them with every entry ON the 5-digit grid, where a - b c lands on exact ties of
    round5.  -> (operand tuples of the final population, their scale estimates)."""
    rng = np.random.default_rng(seed)
    a, b = draw_tuples(rng, pop // 2, "d1"), draw_tuples(rng, pop - pop // 2, "P")
    c = {k: np.concatenate([a[k], b[k]]) for k in a}
    on_grid = rng.random(pop) < 0.5
    c = {k: np.where(on_grid, (np.rint(v.astype(f64) * 1e5) / 1e5).astype(f32), v) for k, v in c.items()}
    best = scale_estimate(c)
    rows = np.arange(pop)
    for _ in range(sweeps):
        for key in ("cjk", "cXk", "cYk", "cXY", "cXj", "cYj"):
            cands = _grid_candidates(c[key], rng, (pop, cand))
            trial = {k: np.repeat(v[:, None], cand, 1).ravel() for k, v in c.items()}
            trial[key] = cands.ravel()
            r = scale_estimate(trial).reshape(pop, cand)
            j = np.argmax(r, 1)
            take = r[rows, j] > best
            c[key] = np.where(take, cands[rows, j], c[key])
            best = np.where(take, r[rows, j], best)
    return c, best


def critical_scale(c, iters=14):
    """Per tuple, the largest scale of dl in [0, 1.5] at which the tuple is a violation for one of the three reciprocals (bisection; every tuple
    at its own midpoint in one vectorised call); 0 where it is none at any scale.  A smaller dl raises the lower bound and relaxes the
    guards Pb, Pc > dl and Nlo > 0, so "violation" is monotone in the scale."""
    ex = exact(**c)
    n = len(c["cXY"])

    def viol(s):
        v = np.zeros(n, bool)
        for u in ULPS:
            v |= violations(ex, screen(ex, rcp_ulp=u, scale=s))
        return v

    lo, hi = np.zeros(n), np.full(n, 1.5)  # a violation at lo (or never), none at hi
    top = viol(hi)
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        v = viol(mid)
        lo, hi = np.where(v, mid, lo), np.where(v, hi, mid)
    return np.where(top, 1.5, lo)


# ---- the fast loop's bookkeeping, and the selection of tests/golden/screen_tuples.json ------------------------------------------------
def fz_sure_range(n_obs, alpha_z=2.5758293035489, n_cond=3):
    """(h2, s2): |stat|^2 above which a test of n_cond conditioning variables is significant at alpha = 0.01 and below which its p lies
    in the normal range (x = |z| / sqrt2 < 26), as fz_seg_body derives them -- to 1e-9, enough to choose inputs."""
    zs = np.sqrt(n_obs - 3.0 - n_cond) / 2.0
    return float(np.tanh(alpha_z / (2.0 * zs)) ** 2), float(np.tanh(26.0 * 0.7071067811865476 / zs) ** 2)


def simulate_fast_loop(ex, sc, segments, n_obs):
    """Which size-3 tests of ONE job the fast loop would skip, from the model's values (a prediction used to choose inputs, never an
    expected value).  segments: [(lo, hi)] rank ranges inside the size-3 enumeration as the host cuts them; a segment is one chunk of
    R = ceil(len / 256) steps, wavefront w owns ranks [lo + 64 R w, lo + 64 R (w + 1)) and tests 64 consecutive ranks per step.  A step is
    skipped when every lane passes the screen against the smallest bound its OWN wavefront has published (what other wavefronts
    published in time is left out: fewer skips, never more); a step evaluated exactly publishes only when every lane is clean, inside
    the sure range and no lane ties with its own best (the commit condition of the fast loop).  -> bool array: skipped."""
    with np.errstate(all="ignore"):
        q = ex["ev"] ** 2 / (ex["xb"] * ex["xc"])
        pub = published(ex)
    h2, s2 = fz_sure_range(n_obs)
    ok = ex["clean"] & ex["f1ok"] & (q > h2) & (q < s2)
    skipped = np.zeros(len(q), bool)
    for lo, hi in segments:
        R = min(-(-(hi - lo) // 256), 64)
        for w in range(4):
            bound, best = f32(np.inf), np.full(64, np.inf)
            for t in range(R):
                r0 = lo + (w * R + t) * 64
                r1 = min(r0 + 64, hi)
                if r0 >= r1:
                    break
                i = np.arange(r0, r1)
                if np.isfinite(bound) and skipped_against_all(sc, i, max(bound, f32(h2 * 1.00001)) * f32(T_FACTOR)):
                    skipped[i] = True
                    continue
                qq, bl = q[i], best[:len(i)]
                take = ~(qq >= bl * (1.0 - 1e-11))
                tie = ~take & (qq <= bl * (1.0 + 1e-11))
                if ok[i].all() and not tie.any() and take.any():
                    bound = min(bound, pub[i][take].min())
                best[:len(i)] = np.where(np.nan_to_num(qq, nan=np.inf) <= bl, qq, bl)
    return skipped


def skipped_against_all(sc, i, T):
    with np.errstate(invalid="ignore", over="ignore"):
        return bool((sc["guards"][i] & (sc["nl2"][i] > f32(T) * sc["den"][i])).all())


TIE_NJ, TIE_NK = 8, 44        # copies of zj / zk in a tie job: accepted = [hub, J_1..8, K_1..44]
TIE_SEGLEN = 2048             # the host's segment length for the batch of tests/test_gpu_fz_screen.py (240 such jobs)
TIE_PARTIALS = ((0.3, 0.3), (0.0, 0.0), (0.6, 0.6), (0.0, 0.6), (0.6, 0.0), (-0.3, 0.3), (0.3, -0.3), (0.85, 0.85))


def tie_job_matrix(t, nj=TIE_NJ, nk=TIE_NK):
    """Matrix over [X, Y, hub, J_1..nj, K_1..nk] around ONE operand tuple t (dict of the ten operands + cJJ, cKK): every J is a copy of
    zj, every K a copy of zk, so each test (hub, J_a, K_b) has exactly the tuple's operands; the copies of zj have cJJ among each other,
    those of zk cKK."""
    p = 3 + nj + nk
    cm = np.eye(p, dtype=f32)
    J, K = np.arange(3, 3 + nj), np.arange(3 + nj, p)

    def put(u, v, x):
        cm[u, v] = f32(x)
        cm[v, u] = f32(x)

    put(0, 1, t["cXY"]), put(0, 2, t["cXz"]), put(1, 2, t["cYz"])
    put(0, J, t["cXj"]), put(1, J, t["cYj"]), put(2, J, t["cjz"])
    put(0, K, t["cXk"]), put(1, K, t["cYk"]), put(2, K, t["ckz"])
    put(J[:, None], K[None, :], t["cjk"])
    cm[np.ix_(J, J)] = np.where(np.eye(nj, dtype=bool), f32(1.0), f32(t["cJJ"]))
    cm[np.ix_(K, K)] = np.where(np.eye(nk, dtype=bool), f32(1.0), f32(t["cKK"]))
    return cm


def tie_job_prediction(t, scale, n_obs=300):
    """-> (the model's rank of the job's maximum-p size-3 test -- the LAST of the smallest |stat|^2 --, would the fast loop skip it with
    dl scaled by `scale`?).  Segments: the job's first window of 256 ranks, then TIE_SEGLEN ranks each."""
    cm = tie_job_matrix(t)
    a = 1 + TIE_NJ + TIE_NK
    ex, sc, _ = job_model(cm, 0, 1, list(range(2, 2 + a)), scale=scale)
    c3 = len(ex["ev"])
    segs = [(0, 256)] + [(lo, lo + TIE_SEGLEN) for lo in range(256, c3 - TIE_SEGLEN + 1, TIE_SEGLEN)]
    with np.errstate(all="ignore"):
        q = ex["ev"] ** 2 / (ex["xb"] * ex["xc"])
    r = int(np.flatnonzero(q == np.nanmin(q))[-1])
    return r, bool(simulate_fast_loop(ex, sc, segs, n_obs)[r])


def select_tie_tuples(oracle_test_subsets, seeds=range(40, 56), sweeps=5, mutant_scale=0.05, min_crit=0.065, n_obs=300):
    """How tests/golden/screen_tuples.json is made.  For each seed: directed_search(seed, sweeps); of its final population the tuples with
    0.04 < |stat|^2 < 0.9 and critical_scale >= min_crit, largest first (at most 60).  For each, the entries among the copies are tried in
    the order of TIE_PARTIALS as partial correlations given the hub (cJJ = cjz^2 + fJ (1 - cjz^2), cKK likewise); the first pair is kept
    for which (a) the oracle (oracle_test_subsets(cm, X, Y, accepted) -> its result) finds the job all-significant with its maximum-p test
    the last tied one, (hub, J_last, K_last), and (b) simulate_fast_loop predicts that test skipped with dl at mutant_scale and not
    skipped at full size.  -> list of dicts (operands, cJJ, cKK)."""
    out = []
    a = 1 + TIE_NJ + TIE_NK
    acc = list(range(2, 2 + a))
    for seed in seeds:
        c, _ = directed_search(seed=seed, sweeps=sweeps)
        ex = exact(**c)
        with np.errstate(all="ignore"):
            q = ex["ev"] ** 2 / (ex["xb"] * ex["xc"])
        cs = critical_scale(c) * ((q < 0.9) & (q > 0.04))
        for i in np.argsort(-cs)[:60]:
            if cs[i] < min_crit:
                break
            t = {k: float(v[i]) for k, v in c.items()}
            cj2, ck2 = float(f32(t["cjz"])) ** 2, float(f32(t["ckz"])) ** 2
            for fJ, fK in TIE_PARTIALS:
                t["cJJ"], t["cKK"] = cj2 + fJ * (1.0 - cj2), ck2 + fK * (1.0 - ck2)
                e = oracle_test_subsets(tie_job_matrix(t), 0, 1, acc)
                if not (e["status"] == 2 and e["Zs"] == (2, 2 + TIE_NJ, 2 + TIE_NJ + TIE_NK)):
                    continue
                if tie_job_prediction(t, mutant_scale, n_obs)[1] and not tie_job_prediction(t, 1.0, n_obs)[1]:
                    out.append(dict(t))
                    break
    return out
