"""The L-BFGS rule of ``qc_lbfgs_step`` restated in numpy from the text of include/qcpinn_hip.h (not from the kernel): both
line-search modes, restart, the resets and the stalled state.  ``dtype`` float64 is the reference; float32 runs the same rule
in the kernel's number format (vector two-loop, numpy's pairwise sums) and gives the tests their measure of fp32 error.
``acc`` (default ``dtype``): the format of the dot products and of the two-loop recursion; float32 vectors with float64
``acc`` is the most an implementation with fp32 vectors can do, and serves the tests as a check that a sequence is
well-posed (its error against float64 is then of the size of the float32 run's, not a multiple of it)."""
import numpy as np

FIXED, ARMIJO = 0, 1


class LbfgsReference:
    def __init__(self, NP, history, line_search=ARMIJO, lr=1.0, c1=1e-4, max_ls=10, shrink_lo=0.1, shrink_hi=0.5,
                 curv_eps=1e-10, dtype=np.float64, acc=None):
        self.NP, self.m, self.mode, self.max_ls = int(NP), int(history), int(line_search), int(max_ls)
        self.dt = np.dtype(dtype).type
        self.acc = self.dt if acc is None else np.dtype(acc).type
        c = self.dt
        self.lr, self.c1, self.lo, self.hi, self.curv_eps = c(lr), c(c1), c(shrink_lo), c(shrink_hi), c(curv_eps)
        self.pairs = []                       # (s, y), oldest first
        self.gamma = c(1.0)
        self.phase = self.n_eval = self.n_iter = self.ls_trials = 0
        self.n_rejected = self.n_skipped_pairs = self.n_resets = self.stalled = self.sd_failed = 0
        self.t = self.f0 = self.gtd0 = self.t_led = c(0.0)
        self.x_k = self.g_k = self.d = None
        self.accepted = 0
        self.rows = []                        # (f, t that led to the point, accepted)
        self.slack = None                     # |f - (f0 + c1 t gtd0)| of the last call when it was an ARMIJO trial,
        self.slack_f0 = None                  # and the f0 it was tested against

    # ---- the pieces of the rule
    def _dot(self, a, b):
        return self.acc(np.dot(a.astype(self.acc), b.astype(self.acc)))

    def _tfirst(self, v):
        with np.errstate(divide="ignore"):
            return self.lr * min(self.dt(1.0), self.dt(1.0) / self.dt(np.abs(v).sum(dtype=self.acc)))

    def _push(self, s, y):
        ys = self._dot(y, s)
        if self.dt(ys) > self.curv_eps:
            if len(self.pairs) == self.m:
                self.pairs.pop(0)
            self.pairs.append((s, y))
            self.gamma = self.dt(ys / self._dot(y, y))
            return True
        return False

    def _dir(self, g):
        A = self.acc
        q = g.astype(A)
        pairs = [(s.astype(A), y.astype(A)) for s, y in self.pairs]
        al = []
        for s, y in reversed(pairs):
            a = A(np.dot(s, q)) / A(np.dot(y, s))
            q = q - a * y
            al.append(a)
        r = A(self.gamma) * q
        for (s, y), a in zip(pairs, reversed(al)):
            b = A(np.dot(y, r)) / A(np.dot(y, s))
            r = r + (a - b) * s
        return (-r).astype(self.dt)

    def _steepest(self, g):
        self.d = -g
        self.t = self._tfirst(g)
        self.gtd0 = -self.dt(self._dot(g, g))

    def restart(self, keep_history):
        self.phase = self.ls_trials = self.stalled = self.sd_failed = 0
        self.t_led = self.dt(0.0)
        if not keep_history:
            self.pairs = []
            self.gamma = self.dt(1.0)

    @property
    def n_pairs(self):
        return len(self.pairs)

    # ---- one call: (params at which f, g were evaluated, f, g) -> the next params
    def step(self, params, f, g):
        c = self.dt
        params, g, f = np.asarray(params, dtype=c), np.asarray(g, dtype=c), c(f)
        self.rows.append((float(f), float(self.t_led), None))
        self.n_eval += 1
        self.slack = None
        out = self._advance(params, f, g)
        self.rows[-1] = (self.rows[-1][0], self.rows[-1][1], self.accepted)
        return out

    def _advance(self, params, f, g):
        c = self.dt
        if self.stalled:
            self.accepted = 0
            self.t_led = c(0.0)
            return self.x_k.copy()
        if self.phase == 0:
            self.phase, self.accepted = 1, 1
            self.n_iter += 1
            self.ls_trials = self.sd_failed = 0
            self.x_k, self.g_k, self.f0 = params.copy(), g.copy(), f
            self._steepest(g)
            self.t_led = self.t
            return self.x_k + self.t * self.d
        if self.mode == FIXED:
            self.accepted = 1
            self.n_iter += 1
            self._push(self.t * self.d, g - self.g_k)
            self.x_k, self.g_k, self.f0 = params.copy(), g.copy(), f
            self.d = self._dir(g)
            self.t = self.lr
            self.gtd0 = c(self._dot(g, self.d))
            if self.gtd0 >= 0:
                self.t_led = c(0.0)
                return params.copy()
            self.t_led = self.t
            return params + self.t * self.d
        # ARMIJO
        with np.errstate(invalid="ignore", over="ignore"):
            bound = self.f0 + self.c1 * self.t * self.gtd0
            finite = bool(np.isfinite(f)) and bool(np.isfinite(g).all())
            self.slack = float(abs(f - bound)) if np.isfinite(f) else float("inf")
            self.slack_f0 = float(self.f0)
            ok = finite and f <= bound
        if ok:
            self.accepted = 1
            self.n_iter += 1
            if not self._push(self.t * self.d, g - self.g_k):
                self.n_skipped_pairs += 1
            self.x_k, self.g_k, self.f0 = params.copy(), g.copy(), f
            self.ls_trials = self.sd_failed = 0
            if not self.pairs:
                self._steepest(g)
            else:
                self.d = self._dir(g)
                self.gtd0 = c(self._dot(g, self.d))
                self.t = self.lr
                if not self.gtd0 < 0:
                    self.pairs = []
                    self.n_resets += 1
                    self._steepest(g)
            self.t_led = self.t
            return self.x_k + self.t * self.d
        self.accepted = 0
        self.n_rejected += 1
        if self.ls_trials + 1 < self.max_ls:
            self.ls_trials += 1
            t = self.t
            with np.errstate(all="ignore"):
                tq = -self.gtd0 * t * t / (c(2.0) * (f - self.f0 - self.gtd0 * t))
            if not np.isfinite(f) or not np.isfinite(tq):
                tq = self.hi * t
            self.t = min(max(tq, self.lo * t), self.hi * t)
            self.t_led = self.t
            return self.x_k + self.t * self.d
        if self.sd_failed and not self.pairs:
            self.stalled = 1
            self.t_led = c(0.0)
            return self.x_k.copy()
        self.n_resets += 1
        self.pairs = []
        self.sd_failed, self.ls_trials = 1, 0
        self._steepest(self.g_k)
        self.t_led = self.t
        return self.x_k + self.t * self.d

    def counters(self):
        return {"n_eval": self.n_eval, "n_iter": self.n_iter, "n_pairs": self.n_pairs, "ls_trials": self.ls_trials,
                "n_rejected": self.n_rejected, "n_skipped_pairs": self.n_skipped_pairs, "n_resets": self.n_resets,
                "stalled": self.stalled, "accepted": self.accepted}


def quartic(N, seed=0, cond=30.0):
    """A convex quartic f(x) = 1/2 sum a_i (x_i - c_i)^2 + 1/4 sum b_i (x_i - c_i)^4 + 1/2 kappa (sum_i u_i (x_i - c_i))^2 (the
    last term couples the coordinates) and its gradient, in float64."""
    rng = np.random.default_rng(seed)
    a = np.exp(rng.uniform(0.0, np.log(cond), N))
    b = rng.uniform(0.5, 2.0, N)
    cc = rng.standard_normal(N)
    u = rng.standard_normal(N) / np.sqrt(N)
    kappa = 5.0

    def fg(x):
        z = np.asarray(x, dtype=np.float64) - cc
        uz = float(u @ z)
        f = 0.5 * float(a @ (z * z)) + 0.25 * float(b @ z ** 4) + 0.5 * kappa * uz * uz
        g = a * z + b * z ** 3 + kappa * uz * u
        return f, g
    return fg
