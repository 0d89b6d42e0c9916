"""A user's own problem as data: collocation points with their targets, and the coefficients of the linear operator

    residual = c_u u + c_t u_t + c_x u_x + c_y u_y - (d_xx u_xx + d_yy u_yy).

The reference's ``Sampler(dim, coords, func)`` (data/diffusion_dataset.py:12-19) accepts ANY callable as the target and
its ``train()`` compares against whatever ``u`` and ``r`` it is handed; the fused HIP step computes only three analytic
targets in-kernel.  A ``TabulatedProblem`` is the general case for that step: the targets are evaluated (or measured)
once, up front, the three segments live on the device, and every training step gathers its minibatch from them on the
device (``qc_sample_dataset``: sampling with replacement, like a ``torch.randint`` minibatch) and reads the targets from
memory (``qc_fused_pinn_data_step``).  ``from_functions`` is the counterpart of ``Sampler(..., func)``.

``coef_res`` makes the operator data too, one row per residual point (``qc_fused_pinn_coef_step``):

    residual_p = c_u[p] u + c_3[p] u^3 + c_t[p] u_t + c_x[p] u_x + c_y[p] u_y - (d_xx[p] u_xx + d_yy[p] u_yy),

rows ``(c_u, c_t, c_x, c_y, d_xx, d_yy, c_3)`` (``COEF_COLUMNS``; ``coef_table`` builds them from scalars, arrays or
callables of X).  A velocity or diffusivity field is a column that varies; a Neumann point is the row
``(0, 0, 1, 0, 0, 0, 0)`` with the prescribed flux as its target; the reference's ``klein_gordon_operator``
(nn/pde.py:28-41) with (t, x) on the x / y slots is ``d_xx=-1, d_yy=-alpha, c_u=beta, c_3=gamma``.  There is no weight
column: a per-point loss weight ``w`` is the row and its target both scaled by ``sqrt(w)``.
"""
from __future__ import annotations

import torch

from .diffusion_dataset import box
from ..hip.lib import QC_ADAPT_FLOOR_MAX, QC_CAUSAL_MAX_SLABS, QC_EQMAX, QC_KMAX, QC_TERMS_MAX

MAX_ROWS = 2 ** 31 - 1      # the device gather forms (32-bit word * rows) >> 32
COEF_COLUMNS = ("c_u", "c_t", "c_x", "c_y", "d_xx", "d_yy", "c_3")     # column order of a coefficient row
COEF_TT_COLUMNS = COEF_COLUMNS + ("d_tt",)      # ... of a row of the seven-channel step (qc_fused_pinn_coef_tt_step)
_SCALARS = {"c_t": 1.0, "c_x": 1.0, "c_y": 1.0, "d_xx": 0.01, "d_yy": 0.01, "c_u": 0.0}


def coef_table(X, **columns):
    """The (N, 7) float32 coefficient table of the points ``X`` (N, 3): each keyword of ``COEF_COLUMNS`` is a scalar, an
    (N,) / (N, 1) array or a callable of X returning one; columns not given are 0."""
    X = torch.as_tensor(X)
    unknown = set(columns) - set(COEF_COLUMNS)
    if unknown:
        raise ValueError(f"unknown coefficient column(s) {sorted(unknown)}: the columns are {COEF_COLUMNS}")
    N = int(X.shape[0])
    out = torch.zeros(N, len(COEF_COLUMNS), dtype=torch.float32)
    for k, name in enumerate(COEF_COLUMNS):
        v = columns.get(name, 0.0)
        if callable(v):
            v = v(X)
        v = torch.as_tensor(v, dtype=torch.float32).cpu()
        if v.dim() > 0:
            v = v.reshape(-1)
            if v.shape[0] != N:
                raise ValueError(f"coefficient column {name}: {N} points but {v.shape[0]} values")
        out[:, k] = v
    return out


def _coef_rows(coef, n_res):
    coef = torch.as_tensor(coef)
    if coef.dtype != torch.float32:
        raise ValueError(f"coefficient table: must be a float32 tensor, got {coef.dtype}")
    if coef.dim() != 2 or coef.shape[1] != len(COEF_COLUMNS):
        raise ValueError(f"coefficient table: must have shape (N, 7) = {COEF_COLUMNS} rows, got {tuple(coef.shape)}")
    if coef.shape[0] != n_res:
        raise ValueError(f"coefficient table: {n_res} residual points but {coef.shape[0]} rows")
    return coef.contiguous()


def _tt_column(d_tt, X_res):
    """The (N_res,) float32 ``d_tt`` column on the device of the residual points: a scalar, an (N_res,) / (N_res, 1)
    float32 tensor or a callable of ``X_res`` returning either."""
    import math
    N = int(X_res.shape[0])
    v = d_tt(X_res) if callable(d_tt) else d_tt
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        if not math.isfinite(float(v)):
            raise ValueError(f"coefficient column d_tt: {v} is not finite")
        return torch.full((N,), float(v), dtype=torch.float32, device=X_res.device)
    v = torch.as_tensor(v)
    if v.dtype != torch.float32:
        raise ValueError(f"coefficient column d_tt: must be a float32 tensor, got {v.dtype}")
    if v.dim() == 0:
        return v.reshape(1).expand(N).to(X_res.device).contiguous()
    if v.dim() > 2 or (v.dim() == 2 and v.shape[1] != 1):
        raise ValueError(f"coefficient column d_tt: must have shape (N,) or (N, 1), got {tuple(v.shape)}")
    v = v.reshape(-1)
    if v.shape[0] != N:
        raise ValueError(f"coefficient column d_tt: {N} points but {v.shape[0]} values")
    if v.device != X_res.device:
        raise ValueError("coefficient column d_tt: must be on the device of the residual points")
    return v.contiguous()


def _segment(name, X, y):
    """(X (N, 3) float32, y (N,) float32) of one segment; an (N, 1) target column is flattened; N = 0 is allowed."""
    X, y = torch.as_tensor(X), torch.as_tensor(y)
    if X.dtype != torch.float32 or y.dtype != torch.float32:
        raise ValueError(f"{name}: points and targets must be float32 tensors, got {X.dtype} and {y.dtype}")
    if X.dim() != 2 or X.shape[1] != 3:
        raise ValueError(f"{name}: points must have shape (N, 3) = (t, x, y) rows, got {tuple(X.shape)}")
    if y.dim() == 2 and y.shape[1] == 1:
        y = y.reshape(-1)
    if y.dim() != 1:
        raise ValueError(f"{name}: targets must have shape (N,) or (N, 1), got {tuple(y.shape)}")
    if y.shape[0] != X.shape[0]:
        raise ValueError(f"{name}: {X.shape[0]} points but {y.shape[0]} targets")
    if X.shape[0] > MAX_ROWS:
        raise ValueError(f"{name}: at most {MAX_ROWS} rows per segment, got {X.shape[0]}")
    return X.contiguous(), y.contiguous()


class LearnedOperator(torch.nn.Module):
    """The operator of an inverse problem: one global coefficient per ``COEF_COLUMNS`` entry, some of them trainable,

        c_k = scale_k * p_k + base_k        (``qc_fused_pinn_inverse_step``; formed with one fused multiply-add).

    ``fixed`` maps a column to its value, ``learn`` maps a column to its initial value, ``scale`` maps a LEARNED column to
    a positive multiplier (default 1); columns not named are fixed at 0.  ``p`` (7,) is the one Parameter and starts at
    0, ``base`` holds the fixed and the initial values, ``scale`` is 0 for a fixed column.  Adam moves every ``p_k`` by
    about ``lr`` per step, so ``scale_k`` is the coefficient's learning-rate multiplier: set it to the magnitude the
    coefficient is expected to have (a diffusivity of 0.01 cannot be learnt in steps of 0.005)."""

    def __init__(self, fixed=None, learn=None, scale=None):
        super().__init__()
        import math
        fixed, learn, scale = dict(fixed or {}), dict(learn or {}), dict(scale or {})
        unknown = (set(fixed) | set(learn) | set(scale)) - set(COEF_COLUMNS)
        if unknown:
            raise ValueError(f"unknown coefficient column(s) {sorted(unknown)}: the columns are {COEF_COLUMNS}")
        both = set(fixed) & set(learn)
        if both:
            raise ValueError(f"column(s) {sorted(both)} are named as fixed and as learned")
        stray = set(scale) - set(learn)
        if stray:
            raise ValueError(f"scale is for learned columns only, got {sorted(stray)}")
        base, sc = [0.0] * len(COEF_COLUMNS), [0.0] * len(COEF_COLUMNS)
        for k, name in enumerate(COEF_COLUMNS):
            v = float(fixed.get(name, learn.get(name, 0.0)))
            if not math.isfinite(v):
                raise ValueError(f"coefficient {name}: {v} is not finite")
            base[k] = v
            if name in learn:
                m = float(scale.get(name, 1.0))
                if not (math.isfinite(m) and m > 0.0):
                    raise ValueError(f"scale of {name}: must be a finite number > 0, got {m}")
                sc[k] = m
        self.p = torch.nn.Parameter(torch.zeros(len(COEF_COLUMNS), dtype=torch.float32))
        self.register_buffer("base", torch.tensor(base, dtype=torch.float32))
        self.register_buffer("scale", torch.tensor(sc, dtype=torch.float32))

    def values(self):
        """(7,) tensor of the effective coefficients: ``base`` where ``scale`` is 0, whatever ``p`` holds."""
        return torch.where(self.scale == 0, self.base, torch.addcmul(self.base, self.scale, self.p.detach()))

    def coefficients(self):
        return {name: float(v) for name, v in zip(COEF_COLUMNS, self.values().cpu())}


class AdaptiveSampling:
    """Residual-adaptive sampling of a dataset's residual rows (RAD / RAR: Wu et al. 2023, Lu et al. 2021): every ``every``
    steps, starting with the first, the residual e_j = |res_j - r_j| is evaluated on ALL residual rows under the current
    parameters, and until the next evaluation the residual batch is drawn with probability proportional to

        e_j^power / mean_i(e_i^power) + floor

    instead of uniformly (``qc_dataset_scores``, ``qc_adapt_build``, ``qc_fused_pinn_adaptive_step``; the exact integer
    rule is in include/qcpinn_hip.h).  ``power`` in 1..4 sharpens the concentration; ``floor`` >= 0 is the share kept for
    uniform coverage (0: proportional to the residual alone, rows of zero residual are then never drawn; 1: about half of
    the batch uniform).  IC and BC rows stay uniform and the loss is not reweighted."""

    def __init__(self, power: int = 1, floor: float = 1.0, every: int = 100):
        if isinstance(power, bool) or not isinstance(power, int) or not 1 <= power <= 4:
            raise ValueError(f"adaptive sampling: power must be an integer in 1..4, got {power!r}")
        floor = float(floor)
        if not (0.0 <= floor <= QC_ADAPT_FLOOR_MAX):
            raise ValueError(f"adaptive sampling: floor must be a finite number in [0, {QC_ADAPT_FLOOR_MAX:g}], got {floor!r}")
        if isinstance(every, bool) or not isinstance(every, int) or every < 1:
            raise ValueError(f"adaptive sampling: every must be a positive integer, got {every!r}")
        self.power, self.floor, self.every = power, floor, every

    def __repr__(self):
        return f"AdaptiveSampling(power={self.power}, floor={self.floor}, every={self.every})"


class CausalWeighting:
    """Causal training of a time-dependent problem (Wang, Sankaran, Perdikaris 2022): the residual points are cut into
    ``n_slabs`` time slabs of equal width and the residual loss becomes

        L_r^c = (1/M) sum_i W_i L_i,      W_i = exp(-eps sum_{k<i} L_k),      W_0 = 1,

    L_i the mean squared residual of the batch's points in slab i, the weights constants when differentiating: a late
    slab counts only once the earlier ones are fitted (``qc_fused_pinn_causal_step``).  ``eps`` is the starting value;
    after every step whose smallest weight W_{M-1} exceeds ``delta`` it is multiplied by ``growth`` up to ``eps_max``.
    ``t_range`` = (t_lo, t_hi) of the slabs (default: the smallest and largest t of the residual points)."""

    def __init__(self, n_slabs: int, eps: float = 1.0, growth: float = 10.0, eps_max: float = 100.0, delta: float = 0.99,
                 t_range=None):
        import math
        if isinstance(n_slabs, bool) or not isinstance(n_slabs, int) or not 2 <= n_slabs <= QC_CAUSAL_MAX_SLABS:
            raise ValueError(f"causal weighting: n_slabs must be an integer in 2..{QC_CAUSAL_MAX_SLABS}, got {n_slabs!r}")
        eps, growth, eps_max, delta = float(eps), float(growth), float(eps_max), float(delta)
        if not (math.isfinite(eps) and eps >= 0.0):
            raise ValueError(f"causal weighting: eps must be a finite number >= 0, got {eps!r}")
        for name, v in (("growth", growth), ("eps_max", eps_max), ("delta", delta)):
            if not (math.isfinite(v) and v > 0.0):
                raise ValueError(f"causal weighting: {name} must be a finite number > 0, got {v!r}")
        if t_range is not None:
            t_range = (float(t_range[0]), float(t_range[1]))
            if not (math.isfinite(t_range[0]) and math.isfinite(t_range[1]) and t_range[0] < t_range[1]):
                raise ValueError(f"causal weighting: t_range must be finite with t_lo < t_hi, got {t_range!r}")
        self.n_slabs, self.eps, self.growth, self.eps_max, self.delta, self.t_range = n_slabs, eps, growth, eps_max, delta, t_range

    def __repr__(self):
        return (f"CausalWeighting(n_slabs={self.n_slabs}, eps={self.eps}, growth={self.growth}, eps_max={self.eps_max}, "
                f"delta={self.delta}, t_range={self.t_range})")

    def edges(self, t):
        """The M + 1 float64 slab edges over ``t_range`` (default: the range of ``t``)."""
        lo, hi = self.t_range if self.t_range is not None else (float(t.min()), float(t.max()))
        if not lo < hi:
            raise ValueError("causal weighting: the residual points span no time interval")
        return torch.linspace(lo, hi, self.n_slabs + 1, dtype=torch.float64)

    def stratify(self, dataset):
        """(sorted, slab_lo): a copy of ``dataset`` whose residual segment is sorted by t (a stable sort: rows of equal t
        keep their order) and the (M + 1,) int64 offsets of the slabs in it.  Slab i holds the rows with edge_i <= t <
        edge_{i+1}; rows below the first edge join slab 0, rows at or above the last edge join slab M - 1.  ValueError on
        an empty slab, on an empty residual segment and on a coefficient table."""
        if dataset.coef_res is not None:
            raise ValueError("causal weighting does not take a per-point coefficient table (dataset.coef_res)")
        if dataset.X_res.shape[0] == 0:
            raise ValueError("causal weighting needs residual points: the dataset's residual segment is empty")
        t = dataset.X_res[:, 0].detach().cpu().double()
        order = torch.sort(t, stable=True).indices
        ts = t[order]
        edges = self.edges(ts)
        lo = torch.searchsorted(ts, edges[1:-1].contiguous(), right=False)      # first row with t >= inner edge
        slab_lo = torch.cat([torch.zeros(1, dtype=torch.int64), lo.to(torch.int64),
                             torch.tensor([ts.numel()], dtype=torch.int64)])
        empty = (slab_lo[1:] - slab_lo[:-1] <= 0).nonzero().reshape(-1).tolist()
        if empty:
            raise ValueError(f"causal weighting: slab(s) {empty} of {self.n_slabs} hold no residual point")
        order = order.to(dataset.X_res.device)
        c = dict(zip(("c_t", "c_x", "c_y", "d_xx", "d_yy"), dataset.coeffs), c_u=dataset.c_u)
        out = TabulatedProblem(dataset.X_res[order].clone(), dataset.r[order].clone(), dataset.X_ic, dataset.u_ic,
                               dataset.X_bc, dataset.u_bc, **c)
        return out, slab_lo


def adaptive_cdf(score, power: int, floor: float):
    """The integer CDF of ``qc_adapt_build`` with torch ops: (N,) float32 scores -> (N,) int64 inclusive sums of
    w_j = q_j + a (the generic training loop draws from it with ``torch.searchsorted``).  torch has no uint64 sums: where
    the device's CDF can pass 2^63 (N (2^24 + a) >= 2^63: more than 2^31 rows at floor 256) this raises ValueError."""
    e = torch.as_tensor(score, dtype=torch.float32).reshape(-1)
    p = e.clone()
    for _ in range(int(power) - 1):
        p = p * e
    p = torch.where(p > 0, p, torch.zeros_like(p)).clamp(max=torch.finfo(torch.float32).max)
    N = p.numel()
    M = p.max()
    if float(M) == 0.0:
        q = torch.ones(N, dtype=torch.int64, device=p.device)
    else:
        s = 23 - (int(torch.frexp(M)[1]) - 1)                  # 23 - ilogb(M)
        q = torch.floor(torch.ldexp(p.double(), torch.tensor(s, device=p.device))).to(torch.int64)
    Q = int(q.sum())
    a = int(float(torch.tensor(floor, dtype=torch.float32)) * float(Q) / float(N))
    if floor > 0 and a == 0:
        a = 1
    if N * (2 ** 24 + a) >= 2 ** 63:
        raise ValueError(f"adaptive sampling: {N} rows at floor {floor} overflow torch's int64 cumulative sum")
    return torch.cumsum(q + a, 0)


class TabulatedProblem:
    """Residual points with forcing values ``r``, initial points with ``u_ic``, boundary points with ``u_bc``."""

    def __init__(self, X_res, r, X_ic, u_ic, X_bc, u_bc, *, c_t=None, c_x=None, c_y=None, d_xx=None, d_yy=None, c_u=None,
                 coef_res=None, d_tt=None):
        """Scalar coefficients (defaults c_t = c_x = c_y = 1, d_xx = d_yy = 0.01, c_u = 0): one operator for every residual
        point.  ``coef_res`` (N_res, 7) float32 instead: one row per residual point; giving it together with any scalar
        coefficient is an error.  ``d_tt`` (beside either): the coefficient of u_tt, a scalar, an (N_res,) float32 tensor or
        a callable of ``X_res``; the problem is then second order in time, ``coef_tt`` is its (N_res, 8) table in
        ``COEF_TT_COLUMNS`` order and training goes through ``qc_fused_pinn_coef_tt_step``.  None: nothing changes."""
        self.X_res, self.r = _segment("residual segment", X_res, r)
        self.X_ic, self.u_ic = _segment("initial segment", X_ic, u_ic)
        self.X_bc, self.u_bc = _segment("boundary segment", X_bc, u_bc)
        given = {k: v for k, v in dict(c_t=c_t, c_x=c_x, c_y=c_y, d_xx=d_xx, d_yy=d_yy, c_u=c_u).items() if v is not None}
        self.coef_res = None
        if coef_res is not None:
            if given:
                raise ValueError(f"coef_res holds the whole operator per point: do not also give {sorted(given)}")
            self.coef_res = _coef_rows(coef_res, self.X_res.shape[0])
            if self.coef_res.device != self.X_res.device:
                raise ValueError("coefficient table: must be on the device of the residual points")
        sc = {**_SCALARS, **given}
        self.coeffs = tuple(float(sc[k]) for k in ("c_t", "c_x", "c_y", "d_xx", "d_yy"))
        self.c_u = float(sc["c_u"])
        self.d_tt = None if d_tt is None else _tt_column(d_tt, self.X_res)

    @property
    def coef_tt(self):
        """The (N_res, 8) float32 operator table in ``COEF_TT_COLUMNS`` order of a problem with ``d_tt``: the rows of
        ``coef_res``, or the scalar coefficients on every row (c_3 = 0), and the ``d_tt`` column; None without ``d_tt``."""
        if self.d_tt is None:
            return None
        if self.coef_res is not None:
            head = self.coef_res
        else:
            c_t, c_x, c_y, d_xx, d_yy = self.coeffs
            head = torch.tensor([self.c_u, c_t, c_x, c_y, d_xx, d_yy, 0.0], dtype=torch.float32,
                                device=self.X_res.device).repeat(self.X_res.shape[0], 1)
        return torch.cat([head, self.d_tt.reshape(-1, 1)], dim=1).contiguous()

    @classmethod
    def from_functions(cls, u_ic, u_bc, r, n_res, n_ic, n_bc, generator=None, coef=None, **coeffs):
        """Evaluate the callables ``u_ic(X)``, ``u_bc(X)``, ``r(X)`` (X: (N, 3) rows (t, x, y) -> (N,) or (N, 1)) on
        uniform points of the trainer's three boxes (trainer/diffusion_train.py:9-20: t = 0 face, x = 0 face, unit cube),
        drawn IC -> BC -> residual from ``generator`` (default: torch's CPU generator).  ``coef``: a callable
        X -> (N, 7) coefficient rows (e.g. ``lambda X: coef_table(X, c_t=1.0, c_x=vx, c_y=vy, ...)``), evaluated on
        the residual points.  ``d_tt`` (among ``coeffs``): as in the constructor; a callable sees the residual points."""
        segs = []
        for name, n, f in (("ics", n_ic, u_ic), ("bc1", n_bc, u_bc), ("dom", n_res, r)):
            b = box(name, "cpu")
            X = b[0:1] + (b[1:2] - b[0:1]) * torch.rand(int(n), 3, generator=generator)
            y = torch.as_tensor(f(X), dtype=torch.float32) if n else torch.zeros(0)
            segs.append((X, y))
        (Xi, ui), (Xb, ub), (Xr, rr) = segs
        if coef is not None:
            coeffs["coef_res"] = torch.as_tensor(coef(Xr), dtype=torch.float32)
        return cls(Xr, rr, Xi, ui, Xb, ub, **coeffs)

    # ---- the three segments in the order the samplers use: residual, IC, BC
    def segments(self):
        return ((self.X_res, self.r), (self.X_ic, self.u_ic), (self.X_bc, self.u_bc))

    def sizes(self):
        return tuple(int(X.shape[0]) for X, _ in self.segments())

    def to(self, device):
        """The same problem with its segments on ``device`` (moved once; a problem already there is returned as is)."""
        device = torch.device(device)
        if all(X.device == device and y.device == device for X, y in self.segments()):
            return self
        c = dict(zip(("c_t", "c_x", "c_y", "d_xx", "d_yy"), self.coeffs), c_u=self.c_u)
        if self.coef_res is not None:
            c = dict(coef_res=self.coef_res.to(device))
        if self.d_tt is not None:
            c["d_tt"] = self.d_tt.to(device)
        (Xr, rr), (Xi, ui), (Xb, ub) = [(X.to(device), y.to(device)) for X, y in self.segments()]
        return TabulatedProblem(Xr, rr, Xi, ui, Xb, ub, **c)


def _system_segment(name, X, Y, width, optional=False):
    """(X (N, 3) float32, Y (N, width) float32 | None) of one segment of a system's dataset; N = 0 is allowed."""
    X = torch.as_tensor(X)
    if X.dtype != torch.float32:
        raise ValueError(f"{name}: points and targets must be float32 tensors, got {X.dtype}")
    if X.dim() != 2 or X.shape[1] != 3:
        raise ValueError(f"{name}: points must have shape (N, 3) = (t, x, y) rows, got {tuple(X.shape)}")
    if X.shape[0] > MAX_ROWS:
        raise ValueError(f"{name}: at most {MAX_ROWS} rows per segment, got {X.shape[0]}")
    if Y is None:
        if not optional:
            raise ValueError(f"{name}: targets are required")
        return X.contiguous(), None
    Y = torch.as_tensor(Y)
    if Y.dtype != torch.float32:
        raise ValueError(f"{name}: points and targets must be float32 tensors, got {X.dtype} and {Y.dtype}")
    if Y.dim() != 2 or Y.shape[1] != width:
        raise ValueError(f"{name}: targets must have shape (N, {width}), got {tuple(Y.shape)}")
    if Y.shape[0] != X.shape[0]:
        raise ValueError(f"{name}: {X.shape[0]} points but {Y.shape[0]} target rows")
    if Y.device != X.device:
        raise ValueError(f"{name}: points and targets must be on one device")
    return X.contiguous(), Y.contiguous()


def check_terms(terms, K, n_eq):
    """The term rows (eq, out, chan, mul0, mul1, coef) of a system as a list of tuples, or ValueError naming the fault:
    the ranges of ``qc_step_system`` (include/qcpinn_hip.h)."""
    import math
    terms = [tuple(t) for t in terms]
    if not 1 <= len(terms) <= QC_TERMS_MAX:
        raise ValueError(f"a system takes 1..{QC_TERMS_MAX} terms, got {len(terms)}")
    out = []
    for i, t in enumerate(terms):
        if len(t) != 6:
            raise ValueError(f"term {i}: expected (eq, out, chan, mul0, mul1, coef), got {t!r}")
        eq, o, ch, m0, m1 = (int(v) for v in t[:5])
        coef = float(t[5])
        if not 0 <= eq < n_eq:
            raise ValueError(f"term {i}: equation {eq} outside 0..{n_eq - 1}")
        if not 0 <= o < K:
            raise ValueError(f"term {i}: output {o} outside 0..{K - 1}")
        if not 0 <= ch <= 5:
            raise ValueError(f"term {i}: channel {ch} outside 0..5 (value, t, x, y, xx, yy)")
        if not (-1 <= m0 < K and -1 <= m1 < K):
            raise ValueError(f"term {i}: multipliers ({m0}, {m1}) must be -1 or an output 0..{K - 1}")
        if not math.isfinite(coef):
            raise ValueError(f"term {i}: coefficient {coef} is not finite")
        out.append((eq, o, ch, m0, m1, coef))
    return out


class TabulatedSystem:
    """A system of equations behind one K-output model as data: residual points with target rows ``R`` (N, n_eq) (None:
    zero), initial and boundary points with the prescribed values ``U`` (N, K) of every output, the operator as a term
    list (rows (eq, out, chan, mul0, mul1, coef), e.g. ``nn.pde.navier_stokes_2D_terms()``), the weights of the equations
    in the residual loss and of the outputs in the value losses (``out_weights[k] = 0``: output k is not prescribed on
    the boundary, e.g. the pressure)."""

    def __init__(self, res, ic, bc, terms, eq_weights=None, out_weights=None):
        import math
        (Xi, Ui), (Xb, Ub) = ic, bc
        if Ui is None:
            raise ValueError("initial segment: targets are required")
        Ui = torch.as_tensor(Ui)
        K = int(Ui.shape[1]) if Ui.dim() == 2 else 0
        if not 1 <= K <= QC_KMAX:
            raise ValueError(f"initial segment: targets must have shape (N, K) with 1 <= K <= {QC_KMAX}, got {tuple(Ui.shape)}")
        Xr, R = res
        if R is not None:
            R = torch.as_tensor(R)
            n_eq = int(R.shape[1]) if R.dim() == 2 else 0
        elif eq_weights is not None:
            n_eq = len(eq_weights)
        else:
            n_eq = 1 + max(int(t[0]) for t in terms)
        if not 1 <= n_eq <= QC_EQMAX:
            raise ValueError(f"a system takes 1..{QC_EQMAX} equations, got {n_eq}")
        self.K, self.n_eq = K, n_eq
        self.X_res, self.R = _system_segment("residual segment", Xr, R, n_eq, optional=True)
        self.X_ic, self.U_ic = _system_segment("initial segment", Xi, Ui, K)
        self.X_bc, self.U_bc = _system_segment("boundary segment", Xb, Ub, K)
        self.terms = check_terms(terms, K, n_eq)
        self.eq_weights = tuple(float(w) for w in (eq_weights if eq_weights is not None else (1.0,) * n_eq))
        self.out_weights = tuple(float(w) for w in (out_weights if out_weights is not None else (1.0,) * K))
        if len(self.eq_weights) != n_eq or len(self.out_weights) != K:
            raise ValueError(f"eq_weights / out_weights must hold {n_eq} / {K} entries, got {len(self.eq_weights)} / "
                             f"{len(self.out_weights)}")
        if not all(math.isfinite(w) for w in self.eq_weights + self.out_weights):
            raise ValueError("eq_weights / out_weights must be finite")

    def segments(self):
        return ((self.X_res, self.R), (self.X_ic, self.U_ic), (self.X_bc, self.U_bc))

    def sizes(self):
        return tuple(int(X.shape[0]) for X, _ in self.segments())

    def to(self, device):
        """The same system with its segments on ``device`` (a system already there is returned as is)."""
        device = torch.device(device)
        if all(X.device == device and (Y is None or Y.device == device) for X, Y in self.segments()):
            return self
        mv = lambda a: None if a is None else a.to(device)
        (Xr, R), (Xi, Ui), (Xb, Ub) = self.segments()
        return TabulatedSystem((mv(Xr), mv(R)), (mv(Xi), mv(Ui)), (mv(Xb), mv(Ub)), self.terms, self.eq_weights,
                               self.out_weights)
