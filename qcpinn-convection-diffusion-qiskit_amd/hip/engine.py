"""Host-side driver of the HIP kernels: owns device workspaces, hands raw pointers and the
current HIP stream to ``libqcpinn_hip.so``.  torch is plumbing here (device memory, streams,
autograd glue); all arithmetic of the hot path runs in the library.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import lib as L
from ..circuits import OP_EMBED_S, GateProgram

NCH = 6  # derivative channels: value, d/dt, d/dx, d/dy, d2/dx2, d2/dy2
NCH_TT = L.QC_NCH_TT  # the same and d2/dt2 as channel 6 (the *_tt entry points)


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _need(t: torch.Tensor, device, what: str) -> torch.Tensor:
    if t.device != device or t.dtype != torch.float32:
        raise L.QcError(f"{what}: expected a float32 tensor on {device}, got {t.dtype} on {t.device}")
    return t.contiguous()


def param_layout(H: int, n: int, n_theta: int, K: int = 1, n_in: int = 3, n_scale: int = 0) -> Dict[str, Tuple[int, Tuple[int, ...]]]:
    """Offsets/shapes of the flat parameter vector = the reference's ``model.parameters()`` order
    (nn/DVPDESolver.py:28-57: preprocessor, postprocessor, quantum_layer); ``K`` outputs: K rows in the last layer;
    ``n_in`` columns of the first layer: 3, or 2 m behind a Fourier-feature map of m frequencies (sines, then cosines).
    ``quantum_layer.params`` spans the whole theta vector of the gate program; its last ``n_scale`` entries, the trainable
    input scalings of a re-uploaded layer, are named once more as ``quantum_layer.embed_scale``."""
    out, off = {}, 0
    for name, shape in (("preprocessor.0.weight", (H, n_in)), ("preprocessor.0.bias", (H,)),
                        ("preprocessor.2.weight", (n, H)), ("preprocessor.2.bias", (n,)),
                        ("postprocessor.0.weight", (H, n)), ("postprocessor.0.bias", (H,)),
                        ("postprocessor.2.weight", (K, H)), ("postprocessor.2.bias", (K,)),
                        ("quantum_layer.params", (n_theta,))):
        out[name] = (off, shape)
        off += int(np.prod(shape))
    out["__total__"] = (off, ())
    if n_scale:
        out["quantum_layer.embed_scale"] = (off - int(n_scale), (int(n_scale),))
    return out


# shapes the network kernels serve (check_mlp in csrc/qc_api.hip); the circuit families alone go to 20 qubits
MLP_MAX_QUBITS = 16
MLP_MAX_HIDDEN = 1024


def check_network_shape(H: int, n: int) -> None:
    """Raise ValueError, naming the limit, for a model the pre/post network kernels cannot run."""
    if not 1 <= int(n) <= MLP_MAX_QUBITS:
        raise ValueError(f"the network kernels (qc_pre_* / qc_post*) serve 1 .. {MLP_MAX_QUBITS} qubits, got {n}: "
                         f"a DVPDESolver takes at most {MLP_MAX_QUBITS} qubits")
    if not 1 <= int(H) <= MLP_MAX_HIDDEN:
        raise ValueError(f"the network kernels (qc_pre_* / qc_post*) serve 1 .. {MLP_MAX_HIDDEN} hidden units, got {H}")


class Circuit:
    """A device-resident gate program + its per-gate trig table and fixed-unitary table."""

    def __init__(self, program: GateProgram, haar: Optional[np.ndarray], device: torch.device,
                 amplitude: bool = False, angle_map: int = L.QC_ANGLE_MAP_NONE):
        if device.type != "cuda":
            raise L.QcError("the HIP kernels need a GPU device (torch device type 'cuda' on ROCm); "
                            "there is no CPU fallback")
        self.lib = L.load()
        self.program = program
        self.device = device
        self.n = program.n_qubits
        self.n_params = program.n_params
        # trainable input scalings of a re-uploaded program (EMBEDS gates): the tail of theta, behind the ansatz slots
        self.n_scale = len({g.slot for g in program.gates if g.op == OP_EMBED_S})
        rows = np.ascontiguousarray(program.rows())
        self.handle = C.c_void_p()
        with torch.cuda.device(device):
            L.check(self.lib.qc_program_create(rows.ctypes.data_as(C.c_void_p), program.n_gates, self.n,
                                               self.n_params, C.byref(self.handle)), "qc_program_create")
        self.amplitude = bool(amplitude)
        if self.amplitude:
            L.check(self.lib.qc_program_set_encoding(self.handle, 1), "qc_program_set_encoding")
        # output map of the pre network in front of this circuit (trainer/train.py: a = pi tanh v); the fused step reads
        # it from the program, the separate entry points from SolverEngine.angle_map
        self.angle_map = int(angle_map)
        if self.angle_map != L.QC_ANGLE_MAP_NONE:
            L.check(self.lib.qc_program_set_angle_map(self.handle, self.angle_map), "qc_program_set_angle_map")
        self.ff_m, self.ff_freq = 0, None      # Fourier-feature input map of the pre network (set_input_map)
        self.trig = torch.zeros(int(self.lib.qc_trig_bytes(self.handle)) // 4, dtype=torch.float32, device=device)
        self.umat = None
        if program.use_haar:
            if haar is None:
                raise L.QcError("program uses the fixed two-wire unitaries but none were given")
            u = np.asarray(haar, dtype=np.complex128)                       # (2,4,4)
            both = np.stack([u, np.conj(np.transpose(u, (0, 2, 1)))], axis=1)  # [slot][fwd|adj][4][4]
            packed = np.stack([both.real, both.imag], axis=-1).astype(np.float32)
            self.umat = torch.from_numpy(np.ascontiguousarray(packed)).to(device)

    @property
    def n_in(self) -> int:
        """Columns of the first layer of the pre network in front of this circuit: 2 m behind an input map, else 3."""
        return 2 * self.ff_m if self.ff_m else 3

    def set_input_map(self, freq) -> None:
        """The Fourier-feature input map gamma(X) = [sin(2 pi X B), cos(2 pi X B)] of the pre network in front of this
        circuit: ``freq`` = B, (3, m) with 1 <= m <= ``QC_FF_MAX`` (rows t, x, y), or None to remove it.  The fused step
        reads it from the program; the separate entry points take the device copy kept here (``ff_freq``)."""
        if freq is None:
            L.check(self.lib.qc_program_set_input_map(self.handle, None, 0), "qc_program_set_input_map")
            self.ff_m, self.ff_freq = 0, None
            return
        B = np.ascontiguousarray(torch.as_tensor(freq).detach().cpu().numpy(), dtype=np.float32)
        if B.ndim != 2 or B.shape[0] != 3 or not 1 <= B.shape[1] <= L.QC_FF_MAX:
            raise ValueError(f"the frequency matrix must be (3, m) with 1 <= m <= {L.QC_FF_MAX}, got {B.shape}")
        with torch.cuda.device(self.device):
            L.check(self.lib.qc_program_set_input_map(self.handle, B.ctypes.data_as(C.c_void_p), B.shape[1]),
                    "qc_program_set_input_map")
        self.ff_m, self.ff_freq = int(B.shape[1]), torch.from_numpy(B).to(self.device)

    def __del__(self):
        try:
            if self.handle:
                self.lib.qc_program_destroy(self.handle)
                self.handle = C.c_void_p()
        except Exception:
            pass

    # -- scratch for the HBM-resident family (n >= 9); empty for the register / lane families
    def workspace(self, nch: int, backward: bool, B: int = 64):
        # the whole batch resident when it fits (fewer, larger launches), never less than the one-tile minimum
        need = max(int(self.lib.qc_circuit_workspace_bytes(self.handle, nch, 1 if backward else 0)),
                   int(self.lib.qc_circuit_workspace_bytes_batch(self.handle, nch, 1 if backward else 0, B)))
        if need == 0:
            return None, 0
        ws = getattr(self, "_ws", None)
        if ws is None or ws.numel() < need:
            self._ws = ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws.data_ptr(), ws.numel()

    # -- parameters changed: refresh cos/sin(theta/2)
    def prepare(self, theta: torch.Tensor) -> None:
        theta = _need(theta.reshape(-1), self.device, "theta")
        L.check(self.lib.qc_prepare_gates(self.handle, theta.data_ptr(), self.trig.data_ptr(),
                                          _stream(self.device)), "qc_prepare_gates")

    # -- amplitude encoding: features -> jets of the normalised initial amplitudes, and back
    def _amp_fwd(self, a: torch.Tensor, nch: int) -> torch.Tensor:
        u = torch.empty_like(a)
        L.check(self.lib.qc_amp_forward(a.data_ptr(), u.data_ptr(), self.n, a.shape[-1], nch, _stream(self.device)),
                "qc_amp_forward")
        return u

    def _amp_bwd(self, a: torch.Tensor, ubar: torch.Tensor, nch: int) -> torch.Tensor:
        ab = torch.empty_like(a)
        L.check(self.lib.qc_amp_backward(a.data_ptr(), ubar.data_ptr(), ab.data_ptr(), self.n, a.shape[-1], nch,
                                         _stream(self.device)), "qc_amp_backward")
        return ab

    def forward_expval(self, angles_nB: torch.Tensor) -> torch.Tensor:
        a = _need(angles_nB, self.device, "angles")
        if self.amplitude:
            a = self._amp_fwd(a, 1)
        B = a.shape[1]
        out = torch.empty_like(a)
        wp, wb = self.workspace(1, False, B)
        L.check(self.lib.qc_forward_expval(self.handle, self.trig.data_ptr(), _ptr(self.umat), a.data_ptr(),
                                           out.data_ptr(), B, wp, wb, _stream(self.device)), "qc_forward_expval")
        return out

    def backward_expval(self, angles_nB: torch.Tensor, cot_nB: torch.Tensor):
        a = _need(angles_nB, self.device, "angles")
        g = _need(cot_nB, self.device, "cotangent")
        return self._adjoint_reduced(a, g, lambda *args: self._adjoint(*args, 1))

    def forward_jets(self, ajets: torch.Tensor) -> torch.Tensor:
        a = _need(ajets, self.device, "angle jets")            # (6, n, B)
        if self.amplitude:
            a = self._amp_fwd(a, NCH)
        B = a.shape[2]
        out = torch.empty_like(a)
        wp, wb = self.workspace(NCH, False, B)
        L.check(self.lib.qc_forward_jets(self.handle, self.trig.data_ptr(), _ptr(self.umat), a.data_ptr(),
                                         out.data_ptr(), B, wp, wb, _stream(self.device)), "qc_forward_jets")
        return out

    def backward_jets(self, ajets: torch.Tensor, qbar: torch.Tensor):
        a = _need(ajets, self.device, "angle jets")
        g = _need(qbar, self.device, "cotangent jets")
        return self._adjoint_reduced(a, g, lambda *args: self._adjoint(*args, NCH))

    def forward_jets_tt(self, ajets: torch.Tensor) -> torch.Tensor:
        """``forward_jets`` on seven channels, (7, n, B) -> (7, n, B) (``qc_forward_jets_tt``: 2 <= n <= 5, angle encoding)."""
        a = _need(ajets, self.device, "angle jets")
        out = torch.empty_like(a)
        L.check(self.lib.qc_forward_jets_tt(self.handle, self.trig.data_ptr(), _ptr(self.umat), a.data_ptr(), out.data_ptr(),
                                            a.shape[2], _stream(self.device)), "qc_forward_jets_tt")
        return out

    def _adjoint_tt(self, a: torch.Tensor, cot: torch.Tensor, part_ptr: int, stride: int) -> torch.Tensor:
        """``_adjoint`` on seven channels (``qc_backward_jets_tt``)."""
        abar = torch.empty_like(a)
        L.check(self.lib.qc_backward_jets_tt(self.handle, self.trig.data_ptr(), _ptr(self.umat), a.data_ptr(), cot.data_ptr(),
                                             abar.data_ptr(), part_ptr, stride, 0, a.shape[-1], _stream(self.device)),
                "qc_backward_jets_tt")
        return abar

    def backward_jets_tt(self, ajets: torch.Tensor, qbar: torch.Tensor):
        """``backward_jets`` on seven channels: (d_ajets (7, n, B), d_theta)."""
        a = _need(ajets, self.device, "angle jets")
        g = _need(qbar, self.device, "cotangent jets")
        return self._adjoint_reduced(a, g, self._adjoint_tt)

    def _adjoint_reduced(self, a: torch.Tensor, cot: torch.Tensor, adjoint):
        """``adjoint(a, cot, part_ptr, stride)`` (``_adjoint`` at a channel count, or ``_adjoint_tt``) on a row matrix of
        its own, and the rows summed: (cotangent of ``a``, d_theta)."""
        B = a.shape[-1]
        rows = (B + 63) // 64
        P = max(self.n_params, 1)
        part = torch.empty(rows, P, dtype=torch.float32, device=self.device)
        abar = adjoint(a, cot, part.data_ptr(), P)
        d_theta = torch.empty(P, dtype=torch.float32, device=self.device)
        L.check(self.lib.qc_reduce_rows(part.data_ptr(), rows, P, P, d_theta.data_ptr(), _stream(self.device)),
                "qc_reduce_rows")
        return abar, d_theta[: self.n_params]

    def _adjoint(self, a: torch.Tensor, cot: torch.Tensor, part_ptr: int, stride: int, nch: int) -> torch.Tensor:
        """Circuit adjoint over the B points of ``a`` (angles [n, B] for nch = 1, angle jets [6, n, B] for nch = 6): returns
        the cotangent of ``a`` and writes one row of d/d(theta) per 64-point tile at ``part_ptr`` (row stride ``stride``)."""
        B = a.shape[-1]
        st = _stream(self.device)
        wp, wb = self.workspace(nch, True, B)
        cin = self._amp_fwd(a, nch) if self.amplitude else a
        abar = torch.empty_like(a)
        fn, name = (self.lib.qc_backward_expval, "qc_backward_expval") if nch == 1 else \
            (self.lib.qc_backward_jets, "qc_backward_jets")
        L.check(fn(self.handle, self.trig.data_ptr(), _ptr(self.umat), cin.data_ptr(), cot.data_ptr(), abar.data_ptr(),
                   part_ptr, stride, 0, B, wp, wb, st), name)
        return self._amp_bwd(a, abar, nch) if self.amplitude else abar


def _pde_record(operator, loss_weights, counts, problem: int, n_seg_a: int) -> "L.QcPde":
    """A ``QcPde``: ``operator`` = its eight floats (D, vx, vy, c_t, c_x, c_y, d_xx, d_yy) as the caller states them, and the
    loss scales of ``loss_weights`` = (residual, BC, IC) over ``counts`` = (residual, IC, BC) points: d loss / d err =
    2 w / N per unit error, 1 / N for the logged means.  Value segment a is the IC points (the first ``n_seg_a``)."""
    w_r, w_bc, w_ic = (float(w) for w in loss_weights)
    n_res, n_ic, n_bc = counts
    return L.QcPde(*operator, 2.0 * w_r / n_res, 1.0 / n_res, 2.0 * w_ic / n_ic, 2.0 * w_bc / n_bc, 1.0 / n_ic, 1.0 / n_bc,
                   problem, n_seg_a)


class SolverEngine:
    """Kernel pipelines of DVPDESolver on one GPU: value forward, residual forward, their reverse
    passes (autograd path), and the fused training step."""

    def __init__(self, circuit: Circuit, hidden: int, flat_params: torch.Tensor,
                 D: float = 0.01, vx: float = 1.0, vy: float = 1.0):
        self.lib = circuit.lib
        self.circuit = circuit
        self.device = circuit.device
        self.n = circuit.n
        self.H = int(hidden)
        check_network_shape(self.H, self.n)
        self.n_theta = circuit.n_params
        # behind an input map the first layer is [H][2m]; the post stage addresses nothing in front of W3, so qc_post* take
        # the flat vector and the gradient rows from `post_shift` entries further on and see their own [H][3] offsets
        self.ff_m = circuit.ff_m
        self.layout = param_layout(self.H, self.n, self.n_theta, n_in=circuit.n_in, n_scale=circuit.n_scale)
        self.post_shift = (circuit.n_in - 3) * self.H
        self.NP = self.layout["__total__"][0]
        self.theta_off = self.layout["quantum_layer.params"][0]
        if flat_params.numel() != self.NP:
            raise L.QcError(f"flat parameter vector has {flat_params.numel()} entries, layout needs {self.NP}")
        self.flat = _need(flat_params, self.device, "flat params")
        self.D, self.vx, self.vy = float(D), float(vx), float(vy)
        self.sigma = (1.0, 1.0, 1.0)                           # sigma_t, sigma_x, sigma_y of nn/pde.py:53-70
        self.coeffs = None      # explicit (c_t, c_x, c_y, d_xx, d_yy) of another linear operator on the same channels
        self.problem = L.QC_PROBLEM_CONVECTION_DIFFUSION      # analytic targets of the fused loss (qcpinn_hip.h)
        self.c_u = 0.0          # zeroth-order coefficient of the residual: the tabulated step only (QC_PROBLEM_TABULATED)
        self.coef_mode = False  # tabulated step with one operator row per residual point (qc_fused_pinn_coef_step)
        self.loss_weights = (2.0, 4.0, 2.0)                    # (residual, BC, IC) weights of the fused loss
        self.angle_map = circuit.angle_map                     # output map of the pre network, on every path
        self._fused: Dict[Tuple[int, int, int], "FusedStep"] = {}

    # ------------------------------------------------------------------ helpers
    def _pde(self, n_res=1, n_ic=1, n_bc=1, n_seg_a=0) -> L.QcPde:
        # loss = 2*MSE_res + 4*MSE_bc + 2*MSE_ic (trainer/diffusion_train.py:47) by default; d/d(err) = 2*w/N * err
        # u_k/sigma_k and u_kk/sigma_k^2 (nn/pde.py:60-70) are scalings of channels the kernels already carry
        st, sx, sy = self.sigma
        co = self.coeffs if self.coeffs is not None else (1.0 / st, self.vx / sx, self.vy / sy, self.D / (sx * sx),
                                                          self.D / (sy * sy))
        return _pde_record((self.D, self.vx, self.vy, *co), self.loss_weights, (n_res, n_ic, n_bc), self.problem, n_seg_a)

    def refresh_gates(self) -> None:
        self.circuit.prepare(self.flat[self.theta_off: self.theta_off + self.n_theta])

    def _post_flat(self) -> int:
        return self.flat.data_ptr() + 4 * self.post_shift

    def _pre_forward(self, X, ajets, B, nch, st) -> None:
        c = self.circuit
        if c.ff_m != self.ff_m:
            raise L.QcError("the circuit's input map changed size after this engine was built")
        if c.ff_m:
            L.check(self.lib.qc_pre_forward_ff(X.data_ptr(), self.flat.data_ptr(), self.H, self.n, self.n_theta, self.angle_map,
                                               c.ff_freq.data_ptr(), c.ff_m, ajets.data_ptr(), B, nch, st), "qc_pre_forward_ff")
            return
        L.check(self.lib.qc_pre_forward_map(X.data_ptr(), self.flat.data_ptr(), self.H, self.n, self.n_theta, self.angle_map,
                                            ajets.data_ptr(), B, nch, st), "qc_pre_forward_map")

    def _pre_backward(self, X, ajets, abar, part, B, nch, st) -> None:
        c = self.circuit
        if c.ff_m:
            L.check(self.lib.qc_pre_backward_ff(X.data_ptr(), self.flat.data_ptr(), self.H, self.n, self.n_theta, self.angle_map,
                                                c.ff_freq.data_ptr(), c.ff_m, ajets.data_ptr(), abar.data_ptr(),
                                                part.data_ptr(), self.NP, 0, B, nch, st), "qc_pre_backward_ff")
            return
        L.check(self.lib.qc_pre_backward_map(X.data_ptr(), self.flat.data_ptr(), self.H, self.n, self.n_theta,
                                             self.angle_map, ajets.data_ptr(), abar.data_ptr(), part.data_ptr(), self.NP, 0,
                                             B, nch, st), "qc_pre_backward_map")

    def _X(self, X: torch.Tensor) -> torch.Tensor:
        X = _need(X, self.device, "collocation points")
        if X.dim() != 2 or X.shape[1] != 3:
            raise L.QcError(f"collocation points must have shape (B, 3), got {tuple(X.shape)}")
        return X

    # ------------------------------------------------------------------ forward passes
    def forward(self, X: torch.Tensor, nch: int, refresh: bool = True, ujets: bool = False):
        """Returns (u, residual_or_None, ajets, qjets).  nch = 1: value only; 6: with residual.  ``ujets`` (nch = 6):
        the first element is the [6, B] tensor of u's derivative channels instead."""
        X = self._X(X)
        B = X.shape[0]
        st = _stream(self.device)
        if refresh:
            self.refresh_gates()
        ajets = torch.empty(nch, self.n, B, dtype=torch.float32, device=self.device)
        self._pre_forward(X, ajets, B, nch, st)
        if nch == 1:
            qjets = self.circuit.forward_expval(ajets[0]).unsqueeze(0)
        else:
            qjets = self.circuit.forward_jets(ajets)
        pde = self._pde()
        if ujets:      # all six derivative channels of u (qc_post mode 4) instead of (u, residual)
            uj = torch.empty(NCH, B, dtype=torch.float32, device=self.device)
            L.check(self.lib.qc_post(4, X.data_ptr(), self._post_flat(), self.H, self.n, self.n_theta,
                                     C.byref(pde), qjets.data_ptr(), uj.data_ptr(), None, None, None, None, None,
                                     0, 0, B, nch, st), "qc_post(forward, six channels)")
            return uj, None, ajets, qjets
        u = torch.empty(B, 1, dtype=torch.float32, device=self.device)
        res = torch.empty(B, 1, dtype=torch.float32, device=self.device) if nch == NCH else None
        L.check(self.lib.qc_post(0, X.data_ptr(), self._post_flat(), self.H, self.n, self.n_theta,
                                 C.byref(pde), qjets.data_ptr(), u.data_ptr(), _ptr(res), None, None, None, None,
                                 0, 0, B, nch, st), "qc_post(forward)")
        return u, res, ajets, qjets

    # ------------------------------------------------------------------ reverse pass (autograd path)
    def backward(self, X, ajets, qjets, ubar, rbar, nch: int, ujets: bool = False) -> torch.Tensor:
        """Vector-Jacobian product of (u, residual) w.r.t. the flat parameters: returns d_flat (NP).  ``ujets``:
        ``ubar`` is the [6, B] cotangent of u's six derivative channels (qc_post mode 3), ``rbar`` unused."""
        X = self._X(X)
        B = X.shape[0]
        pde = self._pde()
        ub = None if ubar is None else _need(ubar.reshape(-1), self.device, "ubar")
        rb = None if (rbar is None or ujets) else _need(rbar.reshape(-1), self.device, "rbar")
        if ujets and (ub is None or ub.numel() != NCH * B or nch != NCH):
            raise L.QcError("the six-channel cotangent must be a [6, B] tensor")
        return self._reverse(
            B, ajets, qjets,
            lambda qbar, part, st: L.check(
                self.lib.qc_post(3 if ujets else 1, X.data_ptr(), self._post_flat(), self.H, self.n, self.n_theta, C.byref(pde),
                                 qjets.data_ptr(), None, None, _ptr(ub), _ptr(rb), qbar.data_ptr(),
                                 part.data_ptr() + 4 * self.post_shift, self.NP, 0, B, nch, st), "qc_post(backward)"),
            lambda *args: self.circuit._adjoint(*args, nch),
            lambda abar, part, st: self._pre_backward(X, ajets, abar, part, B, nch, st))

    def _reduce_rows(self, part: torch.Tensor, st) -> torch.Tensor:
        rows, cols = part.shape
        out = torch.empty(cols, dtype=torch.float32, device=self.device)
        L.check(self.lib.qc_reduce_rows(part.data_ptr(), rows, cols, cols, out.data_ptr(), st), "qc_reduce_rows")
        return out

    def _reverse(self, B, ajets, qjets, post, adjoint, pre_adjoint) -> torch.Tensor:
        """THE reverse pass, over one row of NP entries per 64-point tile: ``post(qbar, part, st)`` fills the cotangent of
        ``qjets`` and the post network's columns, ``adjoint(ajets, qbar, theta columns, stride)`` returns the cotangent of
        ``ajets``, ``pre_adjoint(abar, part, st)`` fills the pre network's columns; returns the rows summed, d_flat (NP)."""
        st = _stream(self.device)
        part = torch.empty((B + 63) // 64, self.NP, dtype=torch.float32, device=self.device)
        qbar = torch.empty_like(qjets)
        post(qbar, part, st)
        abar = adjoint(ajets, qbar, part.data_ptr() + 4 * self.theta_off, self.NP)
        pre_adjoint(abar, part, st)
        return self._reduce_rows(part, st)

    # ------------------------------------------------------------------ seven channels (with d2/dt2)
    def forward_tt(self, X: torch.Tensor, refresh: bool = True):
        """The seven derivative channels of u, (ujets [7, B], ajets [7, n, B], qjets [7, n, B]): value, d/dt, d/dx, d/dy,
        d2/dx2, d2/dy2, d2/dt2 through ``qc_pre_forward_tt``, ``qc_forward_jets_tt`` and ``qc_post_jets_tt`` (2 <= n <= 5,
        angle encoding, no input or angle map: anything else raises ``QcError``)."""
        X = self._X(X)
        B = X.shape[0]
        st = _stream(self.device)
        if self.circuit.ff_m or self.angle_map != L.QC_ANGLE_MAP_NONE:
            raise L.QcError("the seven-channel stages take plain inputs: no Fourier-feature map, no angle map")
        if refresh:
            self.refresh_gates()
        ajets = torch.empty(NCH_TT, self.n, B, dtype=torch.float32, device=self.device)
        L.check(self.lib.qc_pre_forward_tt(X.data_ptr(), self.flat.data_ptr(), self.H, self.n, self.n_theta, ajets.data_ptr(),
                                           B, st), "qc_pre_forward_tt")
        qjets = self.circuit.forward_jets_tt(ajets)
        uj = torch.empty(NCH_TT, B, dtype=torch.float32, device=self.device)
        L.check(self.lib.qc_post_jets_tt(4, self.flat.data_ptr(), self.H, self.n, self.n_theta, qjets.data_ptr(), uj.data_ptr(),
                                         None, None, 0, 0, B, st), "qc_post_jets_tt(forward)")
        return uj, ajets, qjets

    def backward_tt(self, X, ajets, qjets, ubar) -> torch.Tensor:
        """Vector-Jacobian product of the seven channels w.r.t. the flat parameters: ``ubar`` [7, B] -> d_flat (NP)."""
        X = self._X(X)
        B = X.shape[0]
        ub = _need(ubar.reshape(-1), self.device, "ubar").clone()
        if ub.numel() != NCH_TT * B:
            raise L.QcError("the seven-channel cotangent must be a [7, B] tensor")
        return self._reverse(
            B, ajets, qjets,
            lambda qbar, part, st: L.check(
                self.lib.qc_post_jets_tt(3, self.flat.data_ptr(), self.H, self.n, self.n_theta, qjets.data_ptr(), ub.data_ptr(),
                                         qbar.data_ptr(), part.data_ptr(), self.NP, 0, B, st), "qc_post_jets_tt(backward)"),
            self.circuit._adjoint_tt,
            lambda abar, part, st: L.check(
                self.lib.qc_pre_backward_tt(X.data_ptr(), self.flat.data_ptr(), self.H, self.n, self.n_theta, abar.data_ptr(),
                                            part.data_ptr(), self.NP, 0, B, st), "qc_pre_backward_tt"))

    # ------------------------------------------------------------------ K outputs behind one shared network
    def forward_multi(self, X: torch.Tensor, w4k: torch.Tensor):
        """Six derivative channels of every output of a K-output model, [K, 6, B], from ONE pass of pre network,
        circuit and hidden layer (qc_post_multi mode 4).  ``w4k`` = [K, H + 1] rows (W4[k], b4[k]); the W4 / b4 slots of
        the flat vector are unused.  Returns (ujets, ajets, qjets)."""
        X = self._X(X)
        B, K = X.shape[0], int(w4k.shape[0])
        st = _stream(self.device)
        self.refresh_gates()
        w4k = _need(w4k, self.device, "last-layer rows")
        ajets = torch.empty(NCH, self.n, B, dtype=torch.float32, device=self.device)
        self._pre_forward(X, ajets, B, NCH, st)
        qjets = self.circuit.forward_jets(ajets)
        uj = torch.empty(K, NCH, B, dtype=torch.float32, device=self.device)
        L.check(self.lib.qc_post_multi(4, self._post_flat(), self.H, self.n, self.n_theta, K, w4k.data_ptr(),
                                       qjets.data_ptr(), uj.data_ptr(), None, None, None, 0, None, 0, 0, B, st),
                "qc_post_multi(forward)")
        return uj, ajets, qjets

    def backward_multi(self, X, ajets, qjets, w4k, ubar):
        """Reverse of ``forward_multi``: ``ubar`` [K, 6, B] -> (d_flat (NP; zeros in the W4 / b4 slots), d_w4k [K, H + 1]),
        one circuit adjoint sweep and one pre-network reverse pass for all K outputs."""
        X = self._X(X)
        B, K = X.shape[0], int(w4k.shape[0])
        KW = K * (self.H + 1)
        partk = torch.empty((B + 63) // 64, KW, dtype=torch.float32, device=self.device)
        ub = _need(ubar.reshape(-1), self.device, "ubar")
        if ub.numel() != K * NCH * B:
            raise L.QcError("the cotangent must be a [K, 6, B] tensor")
        w4k = _need(w4k, self.device, "last-layer rows")
        d_flat = self._reverse(
            B, ajets, qjets,
            lambda qbar, part, st: L.check(
                self.lib.qc_post_multi(3, self._post_flat(), self.H, self.n, self.n_theta, K, w4k.data_ptr(), qjets.data_ptr(),
                                       None, ub.data_ptr(), qbar.data_ptr(), part.data_ptr() + 4 * self.post_shift, self.NP,
                                       partk.data_ptr(), KW, 0, B, st), "qc_post_multi(backward)"),
            lambda *args: self.circuit._adjoint(*args, NCH),
            lambda abar, part, st: self._pre_backward(X, ajets, abar, part, B, NCH, st))
        return d_flat, self._reduce_rows(partk, _stream(self.device)).view(K, self.H + 1)

    # ------------------------------------------------------------------ fused training step
    def fused(self, B_res: int, n_ic: int, n_bc: int, opt: "OptimState", counts=None) -> "FusedStep":
        key = (B_res, n_ic, n_bc, id(opt), counts, self.problem, self.D, self.vx, self.vy, self.sigma, self.coeffs,
               self.loss_weights, self.c_u, self.coef_mode, self.ff_m)
        if key not in self._fused:
            self._fused[key] = FusedStep(self, B_res, n_ic, n_bc, opt, counts)
        return self._fused[key]


class OptimState:
    """Device-resident Adam moments + the 64-byte {lr, best, num_bad, step, ...} record that the
    optimiser kernel advances (trainer/diffusion_train.py:81-90 without host round trips)."""

    def __init__(self, NP: int, lr: float, device, hist_cap: int = 0, betas=(0.9, 0.999), eps=1e-8,
                 max_norm=1.0, factor=0.9, patience=1000, threshold=1e-4, min_lr=0.0, sched_eps=1e-8,
                 loss_weights=(2.0, 4.0, 2.0)):
        """``max_norm`` None: no gradient clipping (+inf: the kernel's clip coefficient is then 1).  ``loss_weights``:
        (residual, BC, IC) weights of the logged loss (trainer/diffusion_train.py:47 by default)."""
        self.device = device
        self.m = torch.zeros(NP, dtype=torch.float32, device=device)
        self.v = torch.zeros(NP, dtype=torch.float32, device=device)
        rec = np.zeros(16, dtype=np.float32)
        rec[0] = lr
        rec[1] = np.inf                 # ReduceLROnPlateau mode "min": best starts at +inf
        self.state = torch.from_numpy(rec).to(device)
        self.hist = torch.zeros(max(hist_cap, 1), dtype=torch.float32, device=device)
        self.hist_cap = hist_cap
        max_norm = float("inf") if max_norm is None else max_norm
        self.hyper = L.QcOptHyper(betas[0], betas[1], eps, max_norm, factor, threshold, min_lr, sched_eps,
                                  patience, *loss_weights)

    def read(self) -> dict:
        raw = self.state.cpu().numpy()
        ints = raw.view(np.int32)
        return {"lr": float(raw[0]), "best": float(raw[1]), "num_bad_epochs": int(ints[2]), "step": int(ints[3]),
                "hist_base": int(ints[9]),
                "loss": float(raw[4]), "grad_norm": float(raw[5]), "loss_res": float(raw[6]),
                "loss_bc": float(raw[7]), "loss_ic": float(raw[8])}

    def write(self, lr=None, best=None, num_bad=None, step=None, hist_base=None) -> None:
        raw = self.state.cpu().numpy().copy()
        ints = raw.view(np.int32)
        if lr is not None:
            raw[0] = lr
        if best is not None:
            raw[1] = best
        if num_bad is not None:
            ints[2] = num_bad
        if step is not None:
            ints[3] = step
        if hist_base is not None:
            ints[9] = hist_base         # the history buffer starts at this (absolute) step count
        self.state.copy_(torch.from_numpy(raw))

    def loss_history(self, steps: Optional[int] = None):
        """Losses of the first ``steps`` steps of THIS history buffer (default: all taken so far)."""
        if steps is None:
            rec = self.read()
            steps = rec["step"] - rec["hist_base"]
        return self.hist[: max(0, min(steps, self.hist_cap))].cpu().tolist()


LBFGS_LINE_SEARCH = {"fixed": L.QC_LBFGS_FIXED, None: L.QC_LBFGS_FIXED, "armijo": L.QC_LBFGS_ARMIJO}


class LbfgsState:
    """Device-resident L-BFGS state of ``qc_lbfgs_step``: the workspace (128-byte record, x_k, g_k, d, the curvature pairs
    and their Gram entries), the hyper-parameters and the [capacity][3] history (f, t that led to the point, accepted).
    ``advance`` enqueues one call; ``read`` and ``history`` are host reads."""

    _INTS = ("phase", "n_eval", "n_iter", "n_pairs", "head", "ls_trials", "n_rejected", "n_skipped_pairs", "n_resets",
             "stalled", "sd_failed", "NP", "history", "accepted")
    _FLOATS = ("t", "f0", "gtd0", "gamma", "f", "loss_res", "loss_bc", "loss_ic", "t_led")

    def __init__(self, NP: int, device, history: int = 10, line_search="armijo", lr=1.0, c1=1e-4, max_ls=10,
                 shrink_lo=0.1, shrink_hi=0.5, curv_eps=1e-10, loss_weights=(2.0, 4.0, 2.0), capacity: int = 0):
        if line_search not in LBFGS_LINE_SEARCH:
            raise ValueError(f"line_search must be 'armijo', 'fixed' or None, got {line_search!r}")
        self.lib = L.load()
        self.NP, self.m, self.device, self.hist_cap = int(NP), int(history), device, int(capacity)
        need = int(self.lib.qc_lbfgs_workspace_bytes(self.NP, self.m))
        if need == 0:
            raise ValueError(f"L-BFGS needs NP >= 1 and 1 <= history <= {L.QC_LBFGS_MAX_HISTORY}, got NP={NP}, history={history}")
        self.hyper = L.QcLbfgsHyper(self.m, LBFGS_LINE_SEARCH[line_search], int(max_ls), lr, c1, shrink_lo, shrink_hi, curv_eps,
                                    *loss_weights)
        self.ws = torch.empty(need // 4, dtype=torch.float32, device=device)
        self.hist = torch.zeros(max(self.hist_cap, 1), 3, dtype=torch.float32, device=device)
        L.check(self.lib.qc_lbfgs_init(self.ws.data_ptr(), self.NP, self.m, _stream(device)), "qc_lbfgs_init")

    def restart(self, keep_history: bool = False) -> None:
        """The next call is a first evaluation at the current parameters (a new batch)."""
        L.check(self.lib.qc_lbfgs_restart(self.ws.data_ptr(), int(bool(keep_history)), _stream(self.device)), "qc_lbfgs_restart")

    def advance(self, flat: torch.Tensor, params: torch.Tensor, circuit: Optional["Circuit"] = None, theta_off: int = 0) -> None:
        """One ``qc_lbfgs_step``: ``flat`` = [grad[NP] | L_r, L_bc, L_ic] at ``params``; ``params`` receives the next point."""
        prog, trig = (circuit.handle, circuit.trig.data_ptr()) if circuit is not None else (None, None)
        L.check(self.lib.qc_lbfgs_step(flat.data_ptr(), self.NP, params.data_ptr(), self.ws.data_ptr(), C.byref(self.hyper),
                                       self.hist.data_ptr() if self.hist_cap > 0 else None, self.hist_cap, prog, theta_off,
                                       trig, _stream(self.device)), "qc_lbfgs_step")

    def read(self) -> dict:
        raw = self.ws[:L.QC_LBFGS_REC_WORDS].cpu().numpy()
        ints = raw.view(np.int32)
        out = {k: int(ints[i]) for i, k in enumerate(self._INTS)}
        out.update({k: float(raw[16 + i]) for i, k in enumerate(self._FLOATS)})
        return out

    def x_k(self) -> torch.Tensor:
        """The last accepted point (a view of the workspace)."""
        return self.ws[L.QC_LBFGS_REC_WORDS:L.QC_LBFGS_REC_WORDS + self.NP]

    def history(self, n: Optional[int] = None) -> np.ndarray:
        """Rows (f, t, accepted) of the first ``n`` evaluations (default: all so far) that fit the buffer."""
        if n is None:
            n = self.read()["n_eval"]
        return self.hist[: max(0, min(n, self.hist_cap))].cpu().numpy()


class _Step:
    """What every fused step shares: the resident batches ``X_res`` / ``X_val`` (IC points first, then BC) and the stage
    scratch over fixed batch sizes, the per-tile gradient rows ``part`` and their fold ``flat_grad`` ([gradient | L_r, L_bc,
    L_ic], ``stride`` entries), the step workspace, the one ``QcStepDesc`` over them, and the entry point bound once.

    ``flat`` holds the ``param_layout(H, n, n_theta, K)`` entries and the class's ``N_OWN`` trainable entries behind them,
    trained in place; ``what`` names that layout in the size errors (None: the caller has checked)."""

    N_OWN = 0       # trainable entries behind theta (the operator's seven, a balancer's three)
    RES_NCH = NCH   # derivative channels of the residual pipeline's scratch

    def __init__(self, circuit: Circuit, hidden: int, flat: torch.Tensor, opt: OptimState, pde: "L.QcPde", B_res: int,
                 n_ic: int, n_bc: int, K: int = 1, what: Optional[str] = None):
        self.lib, self.circuit, self.opt = circuit.lib, circuit, opt
        dev, n = circuit.device, circuit.n
        self.device, self.n, self.H, self.n_theta = dev, n, int(hidden), circuit.n_params
        check_network_shape(self.H, n)
        self.layout = param_layout(self.H, n, self.n_theta, K, n_in=circuit.n_in, n_scale=circuit.n_scale)     # the step reads the map from the program
        self.NP = self.layout["__total__"][0]
        self.theta_off = self.layout["quantum_layer.params"][0]
        NP_total = self.NP + self.N_OWN
        if what is not None and flat.numel() != NP_total:
            raise L.QcError(f"flat parameter vector has {flat.numel()} entries, {what} needs {NP_total}")
        if what is not None and opt.m.numel() != NP_total:
            raise L.QcError(f"optimiser state holds {opt.m.numel()} entries, {what} needs {NP_total}")
        self.flat = _need(flat, dev, "flat params")
        self.B_res, self.n_ic, self.n_bc = B_res, n_ic, n_bc
        B_val = n_ic + n_bc
        f = dict(dtype=torch.float32, device=dev)
        self.X_res = torch.zeros(max(B_res, 1), 3, **f)
        self.X_val = torch.zeros(max(B_val, 1), 3, **f)
        self.ws_res = torch.empty(4, self.RES_NCH, n, max(B_res, 1), **f)
        self.ws_val = torch.empty(4, 1, n, max(B_val, 1), **f)
        rows = (B_res + 63) // 64 + (B_val + 63) // 64
        self.stride = NP_total + 3
        self.part = torch.zeros(rows, self.stride, **f)
        self.flat_grad = torch.zeros(self.stride, **f)
        self._dataset = None
        c = circuit
        d = L.QcStepDesc()
        d.prog, d.trig_dev, d.umat_dev = c.handle, c.trig.data_ptr(), _ptr(c.umat)
        d.H, d.n, d.n_theta = self.H, n, self.n_theta
        d.params_dev, d.m_dev, d.v_dev = self.flat.data_ptr(), opt.m.data_ptr(), opt.v.data_ptr()
        d.opt_state_dev = opt.state.data_ptr()
        d.hist_dev, d.hist_cap = (opt.hist.data_ptr() if opt.hist_cap > 0 else None), opt.hist_cap
        d.X_res_dev, d.B_res = self.X_res.data_ptr(), B_res
        d.X_val_dev, d.B_val = self.X_val.data_ptr(), B_val
        (d.ajets_res_dev, d.qjets_res_dev, d.qbar_res_dev, d.abar_res_dev) = [self.ws_res[i].data_ptr() for i in range(4)]
        (d.ajets_val_dev, d.qjets_val_dev, d.qbar_val_dev, d.abar_val_dev) = [self.ws_val[i].data_ptr() for i in range(4)]
        d.part_dev, d.part_stride, d.part_rows_cap = self.part.data_ptr(), self.stride, rows
        d.flat_dev = self.flat_grad.data_ptr()
        d.pde = pde
        d.hyper = opt.hyper
        need = int(self.lib.qc_step_workspace_bytes(c.handle, B_res, B_val))
        self.step_ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        d.circ_ws_dev, d.circ_ws_bytes = (self.step_ws.data_ptr(), need) if need else (None, 0)
        d.n_ic = n_ic
        d.comm = None
        d.sample_off_res = d.sample_off_ic = d.sample_off_bc = 0
        d.sample_seed, d.sample_step = 0, 0
        d.sample_bc_face_points = 0
        self.desc = d

    @staticmethod
    def _counts(counts, B_res: int, n_ic: int, n_bc: int):
        """The GLOBAL (residual, IC, BC) point counts the losses are means over (they differ from the local ones under
        data parallelism), at least 1 each."""
        return tuple(max(c, 1) for c in (counts if counts is not None else (B_res, n_ic, n_bc)))

    def _scalar_targets(self, c_u: float) -> None:
        """``target_res`` / ``target_val``, one value per point of the current batches, and the ``QcStepData`` over them
        (the tabulated step and the steps built on it)."""
        f = dict(dtype=torch.float32, device=self.device)
        self.target_res = torch.zeros(max(self.B_res, 1), **f)
        self.target_val = torch.zeros(max(self.n_ic + self.n_bc, 1), **f)
        self.data = L.QcStepData()
        self.data.target_res_dev, self.data.target_val_dev = self.target_res.data_ptr(), self.target_val.data_ptr()
        self.data.c_u = c_u

    def _own_hist(self, cols: int):
        """([max(hist_cap, 1), cols] history of the class's own entries beside the loss history of ``opt``, its address
        for the record or None without a history, hist_cap)."""
        cap = self.opt.hist_cap
        hist = torch.zeros(max(cap, 1), cols, dtype=torch.float32, device=self.device)
        return hist, (hist.data_ptr() if cap > 0 else None), cap

    def _bind_entry(self, name: str, *records) -> None:
        """The export ``run`` calls and its arguments ahead of ``phases``: ``desc`` and the side records (None: a null
        pointer).  Bound once, so that no ``run`` builds a ``byref``; the records are edited in place afterwards."""
        args = (C.byref(self.desc), *(None if r is None else C.byref(r) for r in records))
        self._entry = name, getattr(self.lib, name), args

    def refresh_gates(self) -> None:
        self.circuit.prepare(self.flat[self.theta_off: self.theta_off + self.n_theta])

    def set_sampler(self, seed: int, off_res: int = 0, off_ic: int = 0, off_bc: int = 0,
                    bc_face_points: int = 0) -> None:
        """On-device batches (QC_PHASE_SAMPLE): Philox stream `seed`; off_* = global index of this
        rank's first point in each batch (data parallelism); bc_face_points > 0 spreads the boundary
        batch over the four faces x=0, x=1, y=0, y=1 (that many GLOBAL points per face)."""
        d = self.desc
        d.sample_bc_face_points = bc_face_points
        d.sample_seed = seed & 0xFFFFFFFFFFFFFFFF
        d.sample_off_res, d.sample_off_ic, d.sample_off_bc = off_res, off_ic, off_bc

    def _bind_dataset(self, rec, segments, widths=None, res_optional: bool = False) -> None:
        """Points ``rec`` (a ``QcStepData`` or ``QcStepSystem``: the same ``ds_*`` fields) at the resident dataset
        QC_PHASE_SAMPLE gathers from, ((X_res, r), (X_ic, u_ic), (X_bc, u_bc)) float32 tensors on the step's device, or at
        nothing (None).  ``widths`` None: [N, 3] points and [N] targets per segment; else (N, widths[i]) target rows, which
        the residual segment may go without when ``res_optional``.  An empty segment serves an empty batch only."""
        if segments is None:
            segments = ((None, None),) * 3
        keep = []
        for i, (name, (X, Y)) in enumerate(zip(("res", "ic", "bc"), segments)):
            n = 0 if X is None else int(X.shape[0])
            if n and widths is None:
                X, Y = _need(X, self.device, "dataset points"), _need(Y.reshape(-1), self.device, "dataset targets")
                if X.dim() != 2 or X.shape[1] != 3 or Y.numel() != n:
                    raise L.QcError(f"dataset segment '{name}': points must be (N, 3) with N targets")
            elif n:
                X = _need(X, self.device, "dataset points")
                if X.dim() != 2 or X.shape[1] != 3:
                    raise L.QcError(f"dataset segment '{name}': points must be (N, 3)")
                if Y is not None:
                    Y = _need(Y, self.device, "dataset targets")
                    if tuple(Y.shape) != (n, widths[i]):
                        raise L.QcError(f"dataset segment '{name}': targets must be ({n}, {widths[i]}), got {tuple(Y.shape)}")
                elif name != "res":
                    raise L.QcError(f"dataset segment '{name}': value targets are required")
                elif not res_optional:
                    raise L.QcError("a dataset without residual targets needs a step built with res_targets=False")
            if n:
                keep += [t for t in (X, Y) if t is not None]
            setattr(rec, "ds_X_" + name, X.data_ptr() if n else None)
            setattr(rec, {"res": "ds_r", "ic": "ds_u_ic", "bc": "ds_u_bc"}[name],
                    Y.data_ptr() if n and Y is not None else None)
            setattr(rec, "ds_n_" + name, n)
        self._dataset = keep        # the record holds raw pointers: keep the tensors alive

    def set_dataset(self, segments) -> None:
        """The resident dataset QC_PHASE_SAMPLE gathers from: ((X_res, r), (X_ic, u_ic), (X_bc, u_bc)) float32 tensors on
        the step's device, [N, 3] and [N] per segment (an empty segment serves an empty batch only); None removes it."""
        self._bind_dataset(self.data, segments)

    def set_comm(self, comm) -> None:
        """A communicator of ``qc_comm_create`` (or None): GRADS | UPDATE in one call then all-reduces the flat
        [gradient | 3 loss sums] vector across the ranks inside the library (RCCL, same stream)."""
        self.desc.comm = comm

    def run(self, phases: int = L.QC_PHASE_GRADS | L.QC_PHASE_UPDATE) -> None:
        if phases & L.QC_PHASE_SAMPLE:
            self.desc.sample_step += 1          # a fresh counter block per step
        name, fn, args = self._entry
        L.check(fn(*args, phases, _stream(self.device)), name)


class FusedStep(_Step):
    """One ``qc_fused_pinn_residual_step`` descriptor over fixed-size resident batches.  The caller
    fills ``X_res`` / ``X_val`` (IC points first, then BC points) and calls ``run``.

    When the engine's problem is ``QC_PROBLEM_TABULATED`` the step is ``qc_fused_pinn_data_step``: the caller also fills
    ``target_res`` / ``target_val`` (same order as the points), or hands over a resident dataset with ``set_dataset`` and
    lets ``QC_PHASE_SAMPLE`` gather points and targets from it.  In the engine's coefficient mode (``coef_mode``, tabulated
    only) the step is ``qc_fused_pinn_coef_step``: ``coef_res`` [7][B_res] holds the operator rows of the residual batch
    (c_u, c_t, c_x, c_y, d_xx, d_yy, c_3 per point), filled by the caller or gathered from the dataset's table."""

    def __init__(self, eng: SolverEngine, B_res: int, n_ic: int, n_bc: int, opt: OptimState, counts=None):
        self.eng = eng
        self.tabulated = eng.problem == L.QC_PROBLEM_TABULATED
        self.coef_mode = bool(eng.coef_mode)
        if self.coef_mode and not self.tabulated:
            raise L.QcError("per-point operator rows need the tabulated step (problem = QC_PROBLEM_TABULATED)")
        super().__init__(eng.circuit, eng.H, eng.flat, opt, eng._pde(*self._counts(counts, B_res, n_ic, n_bc), n_ic),
                         B_res, n_ic, n_bc)
        # targets of the current batches and the (optional) resident dataset of the tabulated step
        self._scalar_targets(eng.c_u)
        if self.coef_mode:
            self.coef_res = torch.zeros(L.QC_COEF_COLS, max(B_res, 1), dtype=torch.float32, device=self.device)
            self.coef = L.QcStepCoef()
            self.coef.coef_res_dev, self.coef.ds_coef = (self.coef_res.data_ptr() if B_res else None), None
        self.scores = self.adapt_buf = None
        self.adapt = None       # QcStepAdapt once set_adaptive armed residual-adaptive sampling
        self._bind()

    def set_dataset(self, segments, coef=None) -> None:
        """``_Step.set_dataset``, and ``coef``: the (N_res, 7) float32 operator table beside the residual segment
        (coefficient mode only, where a non-empty residual segment needs it)."""
        if coef is not None and not self.coef_mode:
            raise L.QcError("a coefficient table needs a step in coefficient mode")
        self._bind_dataset(self.data, segments)
        if self.coef_mode:
            n_res = int(self.data.ds_n_res)
            if coef is not None and n_res:
                coef = _need(coef, self.device, "dataset coefficient table")
                if coef.dim() != 2 or tuple(coef.shape) != (n_res, L.QC_COEF_COLS):
                    raise L.QcError(f"dataset coefficient table must be ({n_res}, {L.QC_COEF_COLS}), got {tuple(coef.shape)}")
                self._dataset.append(coef)
                self.coef.ds_coef = coef.data_ptr()
            else:
                self.coef.ds_coef = None
        if self.adapt is not None:      # a CDF belongs to the rows it was built for: a uniform one over the new rows
            self.set_adaptive(self.adapt_power, self.adapt_floor)

    def set_adaptive(self, power: int = 1, floor: float = 1.0) -> None:
        """Residual-adaptive sampling of the dataset's residual rows (after ``set_dataset``): allocates the score tensor
        [ds_n_res] and the CDF buffer, and makes QC_PHASE_SAMPLE draw the residual batch from that CDF
        (``qc_fused_pinn_adaptive_step``).  The CDF starts uniform; ``rescore()`` refreshes it.  A later ``set_dataset``
        re-arms it for the new rows (uniform again until the next ``rescore()``); ``clear_adaptive()`` turns it off."""
        n_rows = int(self.data.ds_n_res)
        if not self.tabulated or n_rows < 1 or self.B_res < 1:
            raise L.QcError("adaptive sampling needs a tabulated step with residual points and a dataset with residual rows")
        self.adapt_power, self.adapt_floor = int(power), float(floor)
        self.scores = torch.zeros(n_rows, dtype=torch.float32, device=self.device)
        need = int(self.lib.qc_adapt_bytes(n_rows))
        self.adapt_buf = torch.zeros((need + 7) // 8, dtype=torch.int64, device=self.device)        # 8-byte aligned
        self.adapt = L.QcStepAdapt(self.adapt_buf.data_ptr(), n_rows)
        self._bind()
        self._build_cdf()       # zero scores: uniform weights

    def clear_adaptive(self) -> None:
        """Back to the uniform gather."""
        self.adapt = self.scores = self.adapt_buf = None
        self._bind()

    def _build_cdf(self) -> None:
        L.check(self.lib.qc_adapt_build(self.scores.data_ptr(), self.adapt.n_rows, self.adapt_power, self.adapt_floor,
                                        self.adapt_buf.data_ptr(), _stream(self.device)), "qc_adapt_build")

    def rescore(self) -> None:
        """Enqueue, on the step's stream, the scores |res - r| of every residual row of the dataset under the current
        parameters and the CDF built from them.  No host read; the step's residual scratch is used between steps."""
        L.check(self.lib.qc_dataset_scores(C.byref(self.desc), C.byref(self.data), C.byref(self.coef) if self.coef_mode else None,
                                           0, self.adapt.n_rows, self.scores.data_ptr(), _stream(self.device)),
                "qc_dataset_scores")
        self._build_cdf()

    def adaptive_state(self) -> dict:
        """The 64-byte record of the CDF buffer (a host read)."""
        raw = self.adapt_buf[:8].cpu().numpy()
        return {"total": int(raw[0]), "q_sum": int(raw[1]), "add": int(raw[2]), "max_p": float(raw[3:4].view(np.float32)[0]),
                "shift": int(raw[3:4].view(np.int32)[1])}

    def _bind(self) -> None:
        """THE place that maps what the step was given (an armed CDF, coefficient mode, a tabulated problem, none of them)
        to one of the four exports and its arguments; re-run when adaptive sampling is (dis)armed."""
        coef = self.coef if self.coef_mode else None
        if self.adapt is not None:
            self._bind_entry("qc_fused_pinn_adaptive_step", self.data, coef, self.adapt)
        elif self.coef_mode:
            self._bind_entry("qc_fused_pinn_coef_step", self.data, coef)
        elif self.tabulated:
            self._bind_entry("qc_fused_pinn_data_step", self.data)
        else:
            self._bind_entry("qc_fused_pinn_residual_step")


class FusedStepTT(FusedStep):
    """One ``qc_fused_pinn_coef_tt_step`` descriptor: the coefficient step with a seventh channel, d2/dt2, for equations
    second order in time over two space dimensions.  The engine's problem must be ``QC_PROBLEM_TABULATED``; ``coef_res``
    [8][B_res] holds the operator rows of the residual batch (c_u, c_t, c_x, c_y, d_xx, d_yy, c_3, d_tt per point), filled
    by the caller or gathered from the dataset's (N_res, 8) table (``set_dataset(segments, coef_tt)``).  2 <= n <= 5, angle
    encoding, no input map, no angle map, no EMBED gates: the library refuses anything else when the step runs."""

    RES_NCH = NCH_TT

    def __init__(self, eng: SolverEngine, B_res: int, n_ic: int, n_bc: int, opt: OptimState, counts=None):
        if eng.problem != L.QC_PROBLEM_TABULATED:
            raise L.QcError("the seven-channel step is a tabulated step (problem = QC_PROBLEM_TABULATED)")
        mode, eng.coef_mode = eng.coef_mode, False      # the 7-column buffers of FusedStep are not this step's
        try:
            super().__init__(eng, B_res, n_ic, n_bc, opt, counts)
        finally:
            eng.coef_mode = mode
        self.coef_res = torch.zeros(L.QC_COEF_TT_COLS, max(B_res, 1), dtype=torch.float32, device=self.device)
        self.coef_tt = L.QcStepCoefTT()
        self.coef_tt.coef_res_dev, self.coef_tt.ds_coef = (self.coef_res.data_ptr() if B_res else None), None
        self._bind()

    def set_dataset(self, segments, coef_tt=None) -> None:
        """``_Step.set_dataset``, and ``coef_tt``: the (N_res, 8) float32 operator table beside the residual segment (a
        non-empty residual segment needs it)."""
        self._bind_dataset(self.data, segments)
        n_res = int(self.data.ds_n_res)
        self.coef_tt.ds_coef = None
        if coef_tt is not None and n_res:
            coef_tt = _need(coef_tt, self.device, "dataset coefficient table")
            if coef_tt.dim() != 2 or tuple(coef_tt.shape) != (n_res, L.QC_COEF_TT_COLS):
                raise L.QcError(f"dataset coefficient table must be ({n_res}, {L.QC_COEF_TT_COLS}), got {tuple(coef_tt.shape)}")
            self._dataset.append(coef_tt)
            self.coef_tt.ds_coef = coef_tt.data_ptr()

    def set_adaptive(self, power: int = 1, floor: float = 1.0) -> None:
        raise L.QcError("the seven-channel step does not support adaptive sampling")

    def _bind(self) -> None:
        if hasattr(self, "coef_tt"):        # (FusedStep's constructor binds before the record exists)
            self._bind_entry("qc_fused_pinn_coef_tt_step", self.data, self.coef_tt)


class SystemStep(_Step):
    """One ``qc_fused_pinn_system_step`` descriptor over fixed-size resident batches: the analogue of ``FusedStep`` for a
    model with K outputs behind one shared network and an operator given as a term list (hip/lib.system_record).

    ``flat`` is the K-row flat parameter vector (``param_layout(H, n, n_theta, K)``), trained in place.  The caller fills
    ``X_res`` / ``X_val`` (IC points first, then BC) and the batch-minor targets ``target_res`` [n_eq, B_res] /
    ``target_val`` [K, B_val], or hands over a resident dataset with ``set_dataset`` and lets ``QC_PHASE_SAMPLE`` gather
    points and target rows.  ``res_targets=False``: the residual targets are zero and no buffer is kept for them."""

    def __init__(self, circuit: Circuit, hidden: int, flat: torch.Tensor, system: "L.QcStepSystem", B_res: int, n_ic: int,
                 n_bc: int, opt: OptimState, counts=None, loss_weights=(2.0, 4.0, 2.0), res_targets: bool = True):
        self.K, self.n_eq = int(system.K), int(system.n_eq)
        if circuit.ff_m:
            raise ValueError("the system step does not serve a pre network behind a Fourier-feature input map")
        if not (1 <= self.K <= L.QC_KMAX and 1 <= self.n_eq <= L.QC_EQMAX):
            raise L.QcError(f"a system has 1..{L.QC_KMAX} outputs and 1..{L.QC_EQMAX} equations, got {self.K} and {self.n_eq}")
        # the operator coefficients and the problem id of the record are not read
        pde = _pde_record((0.0,) * 8, loss_weights, self._counts(counts, B_res, n_ic, n_bc), L.QC_PROBLEM_TABULATED, n_ic)
        super().__init__(circuit, hidden, flat, opt, pde, B_res, n_ic, n_bc, K=self.K, what=f"the {self.K}-output layout")
        f = dict(dtype=torch.float32, device=self.device)
        self.target_res = torch.zeros(self.n_eq, max(B_res, 1), **f) if res_targets else None
        self.target_val = torch.zeros(self.K, max(n_ic + n_bc, 1), **f)
        self.sys = system
        self.sys.target_res_dev = self.target_res.data_ptr() if (res_targets and B_res) else None
        self.sys.target_val_dev = self.target_val.data_ptr()
        self._bind_entry("qc_fused_pinn_system_step", self.sys)

    def set_dataset(self, segments) -> None:
        """The resident dataset QC_PHASE_SAMPLE gathers from: ((X_res, R | None), (X_ic, U_ic), (X_bc, U_bc)) float32
        tensors on the step's device, points [N, 3], target rows [N, n_eq] / [N, K]; None removes it."""
        self._bind_dataset(self.sys, segments, (self.n_eq, self.K, self.K), res_optional=self.target_res is None)


class InverseStep(_Step):
    """One ``qc_fused_pinn_inverse_step`` descriptor over fixed-size resident batches: the tabulated step with a trainable
    global operator c_k = fmaf(scale_k, p_k, base_k), k in ``QC_COEF_COLS`` order.

    ``flat`` holds ``NP + 7`` entries, trained in place: the single-output layout (``param_layout(H, n, n_theta)``) and
    the seven ``p_k`` behind it; ``opt`` holds as many.  ``base`` / ``scale``: seven floats each (``scale_k = 0`` freezes
    a coefficient).  The caller fills ``X_res`` / ``X_val`` (IC points first, then BC) and ``target_res`` / ``target_val``,
    or hands over a resident dataset with ``set_dataset`` and lets ``QC_PHASE_SAMPLE`` gather points and targets.
    ``coef_hist`` [hist_cap, 7] receives the coefficients each step used, beside the loss history of ``opt``."""

    N_OWN = L.QC_COEF_COLS

    def __init__(self, circuit: Circuit, hidden: int, flat: torch.Tensor, base, scale, B_res: int, n_ic: int, n_bc: int,
                 opt: OptimState, counts=None, loss_weights=(2.0, 4.0, 2.0)):
        # the operator is `learn`: the record's own coefficients and data.c_u are poisoned, nothing may read them
        nan = float("nan")
        pde = _pde_record((0.0, 0.0, 0.0, nan, nan, nan, nan, nan), loss_weights, self._counts(counts, B_res, n_ic, n_bc),
                          L.QC_PROBLEM_TABULATED, n_ic)
        super().__init__(circuit, hidden, flat, opt, pde, B_res, n_ic, n_bc, what="the layout with the operator")
        self.NP_L = self.NP + self.N_OWN
        base, scale = [float(v) for v in base], [float(v) for v in scale]
        if len(base) != L.QC_COEF_COLS or len(scale) != L.QC_COEF_COLS:
            raise L.QcError(f"base and scale hold {L.QC_COEF_COLS} entries each")
        self._scalar_targets(nan)
        self.learn = L.QcStepLearn()
        for k in range(L.QC_COEF_COLS):
            self.learn.base[k], self.learn.scale[k] = base[k], scale[k]
        self.coef_hist, self.learn.coef_hist_dev, self.learn.coef_hist_cap = self._own_hist(L.QC_COEF_COLS)
        self._bind_entry("qc_fused_pinn_inverse_step", self.data, self.learn)


class BalancedStep(_Step):
    """One ``qc_fused_pinn_balanced_step`` descriptor over fixed-size resident batches: the tabulated step under learned
    loss weights (uncertainty balancing), F = sum_k (w_k exp(-s_k) L_k + s_k) with s_k = scale_k p_k, k = residual, BC, IC.

    ``flat`` holds ``NP + 3`` entries, trained in place: the single-output layout and the three ``p_k`` behind it; ``opt``
    holds as many.  ``scale``: three floats (``scale_k = 0`` freezes a term at weight w_k).  ``coeffs`` = (c_t, c_x, c_y,
    d_xx, d_yy) and ``c_u``: the operator of the tabulated residual.  Batches, targets and dataset as in ``InverseStep``.
    ``weight_hist`` [hist_cap, 3] receives the effective weights w_k exp(-s_k) each step used, beside the history of F in
    ``opt``."""

    N_OWN = L.QC_BAL_TERMS

    def __init__(self, circuit: Circuit, hidden: int, flat: torch.Tensor, scale, B_res: int, n_ic: int, n_bc: int,
                 opt: OptimState, coeffs, c_u: float = 0.0, counts=None, loss_weights=(2.0, 4.0, 2.0)):
        scale = [float(v) for v in scale]
        if len(scale) != L.QC_BAL_TERMS:
            raise L.QcError(f"scale holds {L.QC_BAL_TERMS} entries: residual, BC, IC")
        pde = _pde_record((0.0, 0.0, 0.0, *(float(c) for c in coeffs)), loss_weights,
                          self._counts(counts, B_res, n_ic, n_bc), L.QC_PROBLEM_TABULATED, n_ic)
        super().__init__(circuit, hidden, flat, opt, pde, B_res, n_ic, n_bc, what="the layout with the operator")
        self.NP_L = self.NP_B = self.NP + self.N_OWN
        self._scalar_targets(float(c_u))
        self.bal = L.QcStepBalance()
        for k in range(L.QC_BAL_TERMS):
            self.bal.scale[k] = scale[k]
        self.weight_hist, self.bal.weight_hist_dev, self.bal.weight_hist_cap = self._own_hist(L.QC_BAL_TERMS)
        self._bind_entry("qc_fused_pinn_balanced_step", self.data, self.bal)


def history_rows(hist: torch.Tensor, steps: Optional[int], cap: int, read, counter: str = "step") -> torch.Tensor:
    """The first ``steps`` rows of the history buffer ``hist`` of ``cap`` rows, on the host.  ``steps`` None: all steps
    of THIS buffer so far, ``read()[counter] - read()["hist_base"]`` of the device record (a host read)."""
    if steps is None:
        rec = read()
        steps = rec[counter] - rec["hist_base"]
    return hist[: max(0, min(int(steps), cap))].cpu()


class _WeightedStep(FusedStep):
    """A ``FusedStep`` with a device record ``state`` of its own (``read_state()``) whose words 2 and 3 are the int32
    counters {n_steps, hist_base} of its history buffer."""

    def set_hist_base(self, n_steps: int, hist_base: int) -> None:
        """Rewrites the two counters of the record (a new history buffer starts at step ``hist_base``)."""
        self.state[2:4] = torch.tensor([n_steps, hist_base], dtype=torch.int32).view(torch.float32).to(self.state.device)

    def _history(self, hist: torch.Tensor, steps: Optional[int], cap: int) -> np.ndarray:
        return history_rows(hist, steps, cap, self.read_state, "n_steps").numpy()


class CausalStep(_WeightedStep):
    """One ``qc_fused_pinn_causal_step`` descriptor over fixed-size resident batches: the tabulated step (the engine's
    problem must be ``QC_PROBLEM_TABULATED``, without coefficient mode) with the residual of time slab i weighted by
    W_i = exp(-eps sum_{k<i} L_k).  ``B_res`` must be a multiple of ``64 * n_slabs``: tile r of the residual batch holds
    points of slab r mod n_slabs, drawn from the dataset's residual segment sorted by t (``set_dataset`` with the sorted
    segments, then ``set_slabs`` with the (M + 1,) int64 offsets of ``data.tabulated.CausalWeighting.stratify``).  Explicit
    batches must be laid out the same way.  ``state`` is the device record {eps, n_raised, n_steps, hist_base, W[M], L[M]};
    ``causal_hist`` [capacity, 1 + 2 M] receives (eps, W, L) of every step."""

    def __init__(self, eng: SolverEngine, B_res: int, n_ic: int, n_bc: int, opt: OptimState, n_slabs: int, eps: float,
                 growth: float, eps_max: float, delta: float, capacity: int = 0, counts=None):
        M = int(n_slabs)
        if not 2 <= M <= L.QC_CAUSAL_MAX_SLABS:
            raise L.QcError(f"n_slabs must lie in 2..{L.QC_CAUSAL_MAX_SLABS}, got {M}")
        if B_res <= 0 or B_res % (64 * M):
            raise L.QcError(f"the causal step needs B_res a positive multiple of 64 * n_slabs = {64 * M}, got {B_res}")
        if eng.problem != L.QC_PROBLEM_TABULATED or eng.coef_mode:
            raise L.QcError("the causal step is the tabulated step without a coefficient table")
        dev = eng.device
        self.n_slabs, self.causal_cap = M, int(capacity)
        self.state = torch.zeros(L.QC_CAUSAL_HEAD + 2 * M, dtype=torch.float32, device=dev)
        self.causal_hist = torch.zeros(max(self.causal_cap, 1), 1 + 2 * M, dtype=torch.float32, device=dev)
        self.slab_lo = None
        self.causal = L.QcStepCausal(M, float(eps), float(growth), float(eps_max), float(delta), None, self.state.data_ptr(),
                                     self.causal_hist.data_ptr() if self.causal_cap > 0 else None, self.causal_cap)
        super().__init__(eng, B_res, n_ic, n_bc, opt, counts)
        L.check(eng.lib.qc_causal_init(self.state.data_ptr(), C.byref(self.causal), _stream(dev)), "qc_causal_init")

    def set_slabs(self, slab_lo) -> None:
        """The (M + 1,) int64 row offsets of the slabs in the dataset's (sorted) residual segment; None removes them."""
        if slab_lo is None:
            self.slab_lo, self.causal.slab_lo_dev = None, None
            return
        t = torch.as_tensor(slab_lo, dtype=torch.int64).reshape(-1).to(self.eng.device).contiguous()
        if t.numel() != self.n_slabs + 1:
            raise L.QcError(f"slab_lo holds n_slabs + 1 = {self.n_slabs + 1} offsets, got {t.numel()}")
        self.slab_lo, self.causal.slab_lo_dev = t, t.data_ptr()

    def set_adaptive(self, power: int = 1, floor: float = 1.0) -> None:
        raise L.QcError("the causal step draws its residual rows by slab: adaptive sampling is not supported")

    def _bind(self) -> None:
        self._bind_entry("qc_fused_pinn_causal_step", self.data, self.causal)

    def read_state(self) -> dict:
        """The record as a dict (a host read): eps of the NEXT step, the counters, W and L of the last step."""
        raw = self.state.cpu().numpy()
        ints, M = raw.view(np.int32), self.n_slabs
        return {"eps": float(raw[0]), "n_raised": int(ints[1]), "n_steps": int(ints[2]), "hist_base": int(ints[3]),
                "W": raw[L.QC_CAUSAL_HEAD:L.QC_CAUSAL_HEAD + M].copy(), "L": raw[L.QC_CAUSAL_HEAD + M:L.QC_CAUSAL_HEAD + 2 * M].copy()}

    def history(self, steps: Optional[int] = None) -> np.ndarray:
        """Rows (eps, W[M], L[M]) of the first ``steps`` steps of the history buffer (default: all taken so far)."""
        return self._history(self.causal_hist, steps, self.causal_cap)


class GradNormStep(_WeightedStep):
    """One ``qc_fused_pinn_gradnorm_step`` descriptor over fixed-size resident batches: the analytic, the tabulated or the
    coefficient step (whichever the engine is configured for, as ``FusedStep``) under gradient-norm loss weights (Wang,
    Teng, Perdikaris 2021): lam_k <- (1 - alpha) lam_k + alpha max|G_res| / mean|G_k| for k = BC, IC every ``every`` steps,
    and the update along G_res + lam_bc G_bc + lam_ic G_ic.  With both value classes present ``n_ic`` must be a multiple
    of 64, so that no 64-point tile of the value batch mixes IC and BC points.  ``state`` is the device record {lam_bc,
    lam_ic, n_steps, hist_base, n_updates, m_r, a_bc, a_ic, hat_bc, hat_ic, 0..}; ``gradnorm_hist`` [capacity, 7] receives
    (lam_bc, lam_ic, m_r, a_bc, a_ic, lambda-weighted loss, updated) of every step."""

    _FLOATS = ("m_r", "a_bc", "a_ic", "hat_bc", "hat_ic")

    def __init__(self, eng: SolverEngine, B_res: int, n_ic: int, n_bc: int, opt: OptimState, alpha: float = 0.1,
                 every: int = 10, lam_max: float = 1e4, init=(1.0, 1.0), capacity: int = 0, counts=None):
        if n_ic > 0 and n_bc > 0 and n_ic % 64:
            raise L.QcError(f"the gradient-norm step needs n_ic a multiple of 64 when IC and BC points are both present, got {n_ic}")
        dev = eng.device
        self.gradnorm_cap = int(capacity)
        self.state = torch.zeros(L.QC_GRADNORM_STATE_WORDS, dtype=torch.float32, device=dev)
        self.gradnorm_hist = torch.zeros(max(self.gradnorm_cap, 1), L.QC_GRADNORM_HIST_COLS, dtype=torch.float32, device=dev)
        self.gn = L.QcStepGradnorm(float(alpha), float(lam_max), int(every), float(init[0]), float(init[1]),
                                   self.state.data_ptr(), self.gradnorm_hist.data_ptr() if self.gradnorm_cap > 0 else None,
                                   self.gradnorm_cap)
        super().__init__(eng, B_res, n_ic, n_bc, opt, counts)
        L.check(eng.lib.qc_gradnorm_init(self.state.data_ptr(), C.byref(self.gn), _stream(dev)), "qc_gradnorm_init")

    def set_adaptive(self, power: int = 1, floor: float = 1.0) -> None:
        raise L.QcError("the gradient-norm step does not support adaptive sampling")

    def _bind(self) -> None:
        self._bind_entry("qc_fused_pinn_gradnorm_step", self.data if self.tabulated else None,
                         self.coef if self.coef_mode else None, self.gn)

    def read_state(self) -> dict:
        """The record as a dict (a host read): the weights of the NEXT step, the counters, the statistics of the last update."""
        raw = self.state.cpu().numpy()
        ints = raw.view(np.int32)
        out = {"lam_bc": float(raw[0]), "lam_ic": float(raw[1]), "n_steps": int(ints[2]), "hist_base": int(ints[3]),
               "n_updates": int(ints[4])}
        out.update({k: float(raw[5 + i]) for i, k in enumerate(self._FLOATS)})
        return out

    def history(self, steps: Optional[int] = None) -> np.ndarray:
        """Rows (lam_bc, lam_ic, m_r, a_bc, a_ic, lambda-weighted loss, updated) of the first ``steps`` steps of the
        history buffer (default: all taken so far)."""
        return self._history(self.gradnorm_hist, steps, self.gradnorm_cap)


def _record_table(records, device) -> torch.Tensor:
    """ctypes records of one type, back to back on the device (a table of ``qc_step_ensemble``)."""
    raw = b"".join(bytes(r) for r in records)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)


class EnsembleStep(_Step):
    """One ``qc_fused_pinn_ensemble_step`` descriptor: M models of one architecture and one gate program trained by one
    launch sequence per step, every launch over the tiles of all members.  Member m computes what a ``FusedStep`` computes
    on its own slices, with the sampler key ``seed + m``.

    ``flats`` / ``opts`` / ``pdes``: every member's flat parameter vector, ``OptimState`` and ``QcPde``.  The step owns
    STACKED copies, one row per member: ``params`` [M, .], ``m`` / ``v``, ``state`` [M, 16], ``hist``, ``trig``, ``X_res``
    [M, .], ``X_val``, the stage scratch, ``part`` [M, rows, stride], ``flat_grad`` [M, .] and the workspaces; a row holds
    the member's slice at its head and ``pad`` more floats behind it (guard bands for tests; 0 otherwise; byte strides are
    rounded up to 256).  Records that differ between members (operator constants and loss weights in ``pdes``, clip norm,
    scheduler settings and loss weights in the ``hyper`` of ``opts``) travel as device tables.  ``member(m)`` is an
    ``OptimState`` over member m's rows; ``read`` / ``write`` / ``loss_history`` go through it."""

    def __init__(self, circuit: Circuit, hidden: int, flats, opts, pdes, B_res: int, n_ic: int, n_bc: int, pad: int = 0):
        M = len(flats)
        if M < 1 or len(opts) != M or len(pdes) != M:
            raise L.QcError("an ensemble needs one flat vector, one optimiser state and one operator record per member")
        super().__init__(circuit, hidden, flats[0], opts[0], pdes[0], B_res, n_ic, n_bc)
        self.M, self.pad = M, int(pad)
        d, dev, lib = self.desc, self.device, self.lib
        ens = L.QcStepEnsemble()
        L.check(lib.qc_ensemble_strides(C.byref(d), M, C.byref(ens)), "qc_ensemble_strides")
        for name in ("params_stride", "flat_stride", "hist_stride", "x_res_stride", "x_val_stride", "jets_res_stride",
                     "jets_val_stride"):
            setattr(ens, name, getattr(ens, name) + self.pad)
        ens.trig_stride = (ens.trig_stride + 4 * self.pad + 255) // 256 * 256
        ens.ws_stride = max((ens.ws_stride + 4 * self.pad + 255) // 256 * 256, 256)
        f = dict(dtype=torch.float32, device=dev)
        NP, cap = self.NP, opts[0].hist_cap
        if any(x.numel() != NP for x in flats) or any(o.m.numel() != NP or o.hist_cap != cap for o in opts):
            raise L.QcError(f"every member needs {NP} parameters and moments and a loss history of {cap} steps")
        self.params = torch.zeros(M, ens.params_stride, **f)
        self.m, self.v = torch.zeros_like(self.params), torch.zeros_like(self.params)
        self.state = torch.zeros(M, 16, **f)
        self.hist = torch.zeros(M, max(ens.hist_stride, 1), **f)
        for k, (x, o) in enumerate(zip(flats, opts)):
            self.params[k, :NP], self.m[k, :NP], self.v[k, :NP] = _need(x, dev, "flat params"), o.m, o.v
            self.state[k] = o.state
            if cap > 0:
                self.hist[k, :cap] = o.hist[:cap]
        self.hypers = [o.hyper for o in opts]
        self.trig = torch.zeros(M, ens.trig_stride // 4, **f)
        self.X_res = torch.zeros(M, ens.x_res_stride, **f)
        self.X_val = torch.zeros(M, ens.x_val_stride, **f)
        self.ws_res = torch.zeros(4, M, ens.jets_res_stride, **f)
        self.ws_val = torch.zeros(4, M, ens.jets_val_stride, **f)
        self.part = torch.zeros(M, int(d.part_rows_cap), self.stride, **f)
        self.flat_grad = torch.zeros(M, ens.flat_stride, **f)
        self.step_ws = torch.zeros(M, ens.ws_stride, dtype=torch.uint8, device=dev)
        d.trig_dev, d.params_dev, d.m_dev, d.v_dev = (t.data_ptr() for t in (self.trig, self.params, self.m, self.v))
        d.opt_state_dev = self.state.data_ptr()
        d.hist_dev = self.hist.data_ptr() if cap > 0 else None
        d.X_res_dev, d.X_val_dev = self.X_res.data_ptr(), self.X_val.data_ptr()
        (d.ajets_res_dev, d.qjets_res_dev, d.qbar_res_dev, d.abar_res_dev) = [self.ws_res[i].data_ptr() for i in range(4)]
        (d.ajets_val_dev, d.qjets_val_dev, d.qbar_val_dev, d.abar_val_dev) = [self.ws_val[i].data_ptr() for i in range(4)]
        d.part_dev, d.flat_dev = self.part.data_ptr(), self.flat_grad.data_ptr()
        d.circ_ws_dev = self.step_ws.data_ptr()
        # the tables, only where the members differ
        self.pdes = list(pdes)
        self.pde_table = self.hyper_table = None
        if any(bytes(p) != bytes(pdes[0]) for p in pdes):
            self.pde_table = _record_table(pdes, dev)
        if any(bytes(h) != bytes(self.hypers[0]) for h in self.hypers):
            self.hyper_table = _record_table(self.hypers, dev)
        ens.pde_dev, ens.hyper_dev = _ptr(self.pde_table), _ptr(self.hyper_table)
        self.ens = ens
        self._bind_entry("qc_fused_pinn_ensemble_step", self.ens)

    def points(self, m: int):
        """(X_res [B_res, 3], X_val [n_ic + n_bc, 3]) of member ``m``: views of its rows."""
        B_val = self.n_ic + self.n_bc
        return self.X_res[m, :3 * self.B_res].view(self.B_res, 3), self.X_val[m, :3 * B_val].view(B_val, 3)

    def member(self, m: int) -> OptimState:
        """An ``OptimState`` over member ``m``'s rows of the stacked moments, state records and loss histories."""
        o = object.__new__(OptimState)
        o.device, o.hyper, o.hist_cap = self.device, self.hypers[m], self.opt.hist_cap
        o.m, o.v, o.state = self.m[m, :self.NP], self.v[m, :self.NP], self.state[m]
        o.hist = self.hist[m, :max(o.hist_cap, 1)]
        return o

    def read(self, m: int) -> dict:
        return self.member(m).read()

    def write(self, m: int, **fields) -> None:
        self.member(m).write(**fields)

    def loss_history(self, m: int, steps: Optional[int] = None):
        return self.member(m).loss_history(steps)

    def refresh_gates(self) -> None:
        st = _stream(self.device)
        for m in range(self.M):
            theta = self.params[m, self.theta_off: self.theta_off + self.n_theta]
            L.check(self.lib.qc_prepare_gates(self.circuit.handle, theta.data_ptr(), self.trig[m].data_ptr(), st),
                    "qc_prepare_gates")

    def set_comm(self, comm) -> None:
        if comm is not None:
            raise L.QcError("an ensemble step is single-process: it takes no communicator")
