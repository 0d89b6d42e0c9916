"""Shared by the L-BFGS GPU tests: a device-side driver of ``qc_lbfgs_step`` on padded buffers, the float64 / float32
reference pair fed the same values, and the scripted (f, g) sequences that force every branch of the backtracking mode."""
import ctypes as C

import numpy as np
import torch

import lbfgs_reference as LR
from conftest import pkg

SENTINEL = -777.25
GUARD = 64
W = (2.0, 4.0, 2.0)                     # loss weights of f


def parts_of(f):
    """(L_r, L_bc, L_ic) in float32 whose 2, 4, 2 weighted sum is about ``f``; non-finite f goes to L_r."""
    if not np.isfinite(f):
        return np.array([f, 0.0, 0.0], np.float32)
    return np.array([0.25 * f, 0.0625 * f, 0.125 * f], np.float32)


def f_of(parts):
    """The float64 value of the weighted sum of float32 parts: what every reference is fed."""
    p = np.asarray(parts, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return W[0] * p[0] + W[1] * p[1] + W[2] * p[2]


class Device:
    """flat / params with GUARD sentinels behind them, an LbfgsState, and one qc_lbfgs_step per ``call``."""

    def __init__(self, NP, x0, device, history, line_search, capacity=256, circuit=None, theta_off=0, **kw):
        E = pkg("hip.engine")
        self.NP, self.device, self.circuit, self.theta_off = NP, device, circuit, theta_off
        self.st = E.LbfgsState(NP, device, history=history, line_search=line_search, loss_weights=W, capacity=capacity, **kw)
        self.flat = torch.full((NP + 3 + GUARD,), SENTINEL, device=device)
        self.prm = torch.full((NP + GUARD,), SENTINEL, device=device)
        self.prm[:NP] = torch.from_numpy(np.asarray(x0, np.float32)).to(device)

    def params(self):
        return self.prm[:self.NP].cpu().numpy()

    def call(self, parts, g):
        vec = np.concatenate([np.asarray(g, np.float32), np.asarray(parts, np.float32)])
        self.flat[:self.NP + 3] = torch.from_numpy(vec).to(self.device)
        self.st.advance(self.flat, self.prm, self.circuit, self.theta_off)
        return self.params()

    def assert_guards(self):
        for name, t, n in (("flat", self.flat, self.NP + 3), ("prm", self.prm, self.NP)):
            tail = t[n:].cpu().numpy()
            assert np.array_equal(tail.view(np.int32), np.full(tail.size, SENTINEL, np.float32).view(np.int32)), name


class RefPair:
    """The reference in float64 and in float32 on one sequence of (f, g); each keeps its own parameters.  ``mixed``: a third
    run, float32 vectors with float64 dot products, for the well-posedness condition of the scripted sequences."""

    def __init__(self, NP, x0, history, line_search, mixed=False, **kw):
        mode = {"fixed": LR.FIXED, None: LR.FIXED, "armijo": LR.ARMIJO}[line_search]
        self.r64 = LR.LbfgsReference(NP, history, mode, dtype=np.float64, **kw)
        self.r32 = LR.LbfgsReference(NP, history, mode, dtype=np.float32, **kw)
        self.rmx = LR.LbfgsReference(NP, history, mode, dtype=np.float32, acc=np.float64, **kw) if mixed else None
        self.x64 = np.asarray(x0, np.float32).astype(np.float64)
        self.x32 = np.asarray(x0, np.float32).copy()
        self.xmx = self.x32.copy()
        self.mixed_err = 0.0

    def step(self, parts, g):
        f, g = f_of(parts), np.asarray(g, np.float32)
        with np.errstate(all="ignore"):
            self.x64 = self.r64.step(self.x64, f, g.astype(np.float64))
            self.x32 = self.r32.step(self.x32, np.float32(f), g)
            if self.rmx is not None:
                self.xmx = self.rmx.step(self.xmx, np.float32(f), g)
                self.mixed_err = float(np.abs(self.xmx.astype(np.float64) - self.x64).max())
        return float(np.abs(self.x32.astype(np.float64) - self.x64).max())

    def restart(self, keep):
        for r in (self.r64, self.r32, self.rmx):
            if r is not None:
                r.restart(keep)


def slack_ok(ref):
    """The condition on the inputs: at an ARMIJO trial with a finite loss the reference's |f - (f0 + c1 t gtd0)| is at least
    1e-3 max(1, |f0|), so fp32 rounding cannot flip the decision."""
    return ref.slack is None or ref.slack >= 1e-3 * max(1.0, abs(ref.slack_f0))


def scripted(NP, history, script, seed, max_ls=10, jump=3.0, cond=20.0, **kw):
    """(parts, g) per evaluation for the backtracking mode, planned with a float64 reference so that every call takes the
    branch its letter names.  The list does not depend on the parameters of whoever is fed it, so the device and both
    references see the same values.  Gradients are those of a quadratic 1/2 (x - c)' A (x - c), A diagonal with entries in
    [1, cond], at the planner's own trial points (NP < history: a fresh A at every accepted point, since more pairs of ONE quadratic than
    dimensions make the recursion ill-conditioned in any precision); its centre c jumps at every accepted point by ``jump`` along a direction
    A-orthogonal to s (so y.s = s'As > 0 and the gradients never die out).  Losses are scripted:
      F first evaluation        A accepted, pair kept        S accepted, pair skipped (y.s < 0)
      Z accepted with g = 0: the new direction is no descent direction (reset)
      Q rejected, t_q = 0.3 t   C rejected, t_q = 0.02 t (clamped to shrink_lo t)
      N rejected, loss NaN      I rejected, one gradient entry +inf (loss at the accepted level)
      R / K restart without / with the history (no evaluation; the next letter must be F)
    Accepted losses lie 0.05 max(1, |f0|) below the Armijo bound; rejected ones |gtd0| t (2/3 or 24) above f0.
    Returns (list of ("eval", parts, g) / ("restart", keep), the planner)."""
    rng = np.random.default_rng(seed)
    ref = LR.LbfgsReference(NP, history, LR.ARMIJO, max_ls=max_ls, **kw)
    A = np.exp(rng.uniform(0.0, np.log(cond), NP))
    x = rng.standard_normal(NP)             # the planner's own current point
    c = x + jump * rng.standard_normal(NP) / np.sqrt(NP)
    out = []

    def a_perp(v):
        """unit vector u with u'Av = 0"""
        u = rng.standard_normal(NP)
        av = A * v
        n2 = float(av @ av)
        if n2 > 0 and NP > 1:
            u = u - (u @ av) / n2 * av
        n = np.linalg.norm(u)
        return u / n if n > 0 else u

    for letter in script:
        if letter in "RK":
            ref.restart(letter == "K")
            out.append(("restart", letter == "K"))
            continue
        if letter == "F":
            g = A * (x - c)
            f = 10.0 if ref.n_eval == 0 else float(ref.f0) - 1.0
        else:
            f0, t, gtd0 = float(ref.f0), float(ref.t), float(ref.gtd0)
            s = t * ref.d
            if letter in "ASZ" and NP < history:
                A = np.exp(rng.uniform(0.0, np.log(cond), NP))      # fewer dimensions than pairs: no common Hessian
            c = ref.x_k - ref.g_k / A           # the quadratic whose gradient at x_k is g_k
            f_acc = f0 + float(ref.c1) * t * gtd0 - 0.05 * max(1.0, abs(f0))
            g = A * (x - c)
            if letter == "A":
                f = f_acc
                g = A * (x - (c + jump * a_perp(s)))
            elif letter == "S":
                f, g = f_acc, ref.g_k - 0.1 * np.linalg.norm(ref.g_k) / np.linalg.norm(s) * s
            elif letter == "Z":
                f, g = f_acc, np.zeros(NP)
            elif letter == "Q":
                f = f0 + gtd0 * t * (1.0 - 1.0 / 0.6)
            elif letter == "C":
                f = f0 + gtd0 * t * (1.0 - 25.0)
            elif letter == "N":
                f = float("nan")
            elif letter == "I":
                f = f_acc
                g[int(rng.integers(NP))] = np.inf
            else:
                raise ValueError(letter)
        parts = parts_of(f)
        g32 = np.asarray(g, np.float32)
        with np.errstate(all="ignore"):
            x = ref.step(x, f_of(parts), g32.astype(np.float64))
        out.append(("eval", parts, g32))
    return out, ref
