"""The tabulated step without a GPU: the three new exports and their argument refusals, TabulatedProblem, the index
draw of the device gather restated in numpy, the float64 step reference with targets as arrays (and that its negative
controls differ from it by far more than the GPU tolerance), and train(..., dataset=) on a classical torch model."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

import tabulated_reference as T
from conftest import pkg
from step_reference import haar_for, reference_loss, step_inputs

TOL_G, TOL_L = 2e-4, 1e-4          # the GPU tests' tolerances (tests/test_gpu_fused_families.py)


# ---- 1. ABI
def test_exports_load_and_step_data_matches_the_header_layout():
    L = pkg("hip.lib")
    lib = L.load()
    for name in ("qc_post_data", "qc_sample_dataset", "qc_fused_pinn_data_step"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert L.QC_PROBLEM_TABULATED == 3
    # two pointers, a float (padded to 8), then three (pointer, pointer, int64) triples
    assert C.sizeof(L.QcStepData) == 2 * 8 + 8 + 3 * 24 == 96
    assert L.QcStepData.c_u.offset == 16 and L.QcStepData.ds_X_res.offset == 24 and L.QcStepData.ds_n_bc.offset == 88


def _desc(L, problem, B_res, n_ic, n_bc):
    """A descriptor whose pointers are non-null but never dereferenced: every call below must be refused on the host."""
    d = L.QcStepDesc()
    fake = 4096
    for name, _ in L.QcStepDesc._fields_:
        if name.endswith("_dev") and name != "umat_dev":
            setattr(d, name, fake)
    d.prog = None
    d.H, d.n, d.n_theta = 50, 4, 12
    d.B_res, d.B_val, d.n_ic = B_res, n_ic + n_bc, n_ic
    d.part_stride, d.part_rows_cap = 10 ** 4, 64
    d.pde.problem = problem
    return d


def test_argument_errors_do_not_need_a_gpu():
    L = pkg("hip.lib")
    lib = L.load()
    fake = 4096
    full = L.QcStepData(fake, fake, 0.0, fake, fake, 10, fake, fake, 10, fake, fake, 10)
    pde = L.QcPde()
    pde.problem = L.QC_PROBLEM_TABULATED
    # qc_post_data: no target buffer; a problem id other than 3
    args = (fake, 50, 4, 12, C.byref(pde), fake)
    tail = (fake, fake, fake, fake, 10 ** 4, 0, 64, 6, None)
    assert lib.qc_post_data(*args, None, 0.0, *tail) == -1
    pde.problem = L.QC_PROBLEM_CONVECTION_DIFFUSION
    assert lib.qc_post_data(*args, fake, 0.0, *tail) == -1
    # qc_post keeps refusing id 3
    pde.problem = L.QC_PROBLEM_TABULATED
    assert lib.qc_post(2, fake, fake, 50, 4, 12, C.byref(pde), fake, fake, fake, None, None, fake, fake, 10 ** 4, 0, 64, 6,
                       None) == -1
    # qc_sample_dataset: absent data, missing batch buffers, absent / empty / oversized segments
    call = lambda t, Xr=fake, tr=fake, Xv=fake, tv=fake, n=(5, 3, 2): lib.qc_sample_dataset(
        Xr, tr, n[0], 0, Xv, tv, n[1], 0, n[2], 0, None if t is None else C.byref(t), 1, 1, None)
    assert call(None) == -1
    assert call(full, tr=None) == -1 and call(full, tv=None) == -1 and call(full, Xr=None) == -1
    for field, bad in (("ds_n_res", 0), ("ds_n_ic", 0), ("ds_n_bc", 0), ("ds_n_res", 2 ** 31), ("ds_n_bc", 2 ** 31),
                       ("ds_X_ic", None), ("ds_r", None), ("ds_u_bc", None)):
        t = L.QcStepData(fake, fake, 0.0, fake, fake, 10, fake, fake, 10, fake, fake, 10)
        setattr(t, field, bad)
        assert call(t) == -1, field
    # qc_fused_pinn_data_step: absent data; a problem id other than 3; a missing target buffer; QC_PHASE_SAMPLE without a
    # dataset segment or with one of 2^31 rows.  The entry checks its data before it looks at the program, so these are
    # the refusals of the data check; a program needs a device, so the descriptor's is null and a call that passed the
    # data check would be refused all the same: tests/test_gpu_tabulated.py::test_refusals_name_one_fault_each repeats
    # them on a descriptor that runs but for the one fault named.  The old entry keeps refusing id 3.
    d = _desc(L, L.QC_PROBLEM_TABULATED, 5, 3, 2)
    both = L.QC_PHASE_GRADS | L.QC_PHASE_SAMPLE
    assert lib.qc_fused_pinn_data_step(C.byref(d), None, L.QC_PHASE_GRADS, None) == -1
    assert lib.qc_fused_pinn_residual_step(C.byref(d), L.QC_PHASE_GRADS, None) == -1
    for pb in (0, 1, 2, 4, -1):
        d.pde.problem = pb
        assert lib.qc_fused_pinn_data_step(C.byref(d), C.byref(full), L.QC_PHASE_GRADS, None) == -1
    d.pde.problem = L.QC_PROBLEM_TABULATED
    for field, bad, phases in (("target_res_dev", None, L.QC_PHASE_GRADS), ("target_val_dev", None, L.QC_PHASE_GRADS),
                               ("ds_n_res", 0, both), ("ds_X_bc", None, both), ("ds_n_ic", 2 ** 31, both)):
        t = L.QcStepData(fake, fake, 0.0, fake, fake, 10, fake, fake, 10, fake, fake, 10)
        setattr(t, field, bad)
        assert lib.qc_fused_pinn_data_step(C.byref(d), C.byref(t), phases, None) == -1, field


# ---- 2. TabulatedProblem
def _segments(n_res=5, n_ic=3, n_bc=2):
    g = torch.Generator().manual_seed(0)
    return [torch.rand(n, 3, generator=g) for n in (n_res, n_ic, n_bc)], [torch.rand(n, generator=g) for n in (n_res, n_ic, n_bc)]


def test_tabulated_problem_validates_its_segments():
    TP = pkg("data.tabulated").TabulatedProblem
    (Xr, Xi, Xb), (r, ui, ub) = _segments()
    p = TP(Xr, r, Xi, ui[:, None], Xb, ub, c_u=0.5, d_xx=0.03)
    assert p.sizes() == (5, 3, 2) and p.u_ic.shape == (3,) and p.c_u == 0.5
    assert p.coeffs == (1.0, 1.0, 1.0, 0.03, 0.01)
    assert p.to("cpu") is p
    with pytest.raises(ValueError, match=r"shape \(N, 3\)"):
        TP(Xr[:, :2], r, Xi, ui, Xb, ub)
    with pytest.raises(ValueError, match="float32"):
        TP(Xr.double(), r, Xi, ui, Xb, ub)
    with pytest.raises(ValueError, match="float32"):
        TP(Xr, r, Xi, ui, Xb, ub.double())
    with pytest.raises(ValueError, match="5 points but 3 targets"):
        TP(Xr, ui, Xi, ui, Xb, ub)
    with pytest.raises(ValueError, match="targets must have shape"):
        TP(Xr, torch.stack([r, r], 1), Xi, ui, Xb, ub)
    # empty segments are data too
    e = TP(Xr, r, Xi[:0], ui[:0], Xb[:0], ub[:0])
    assert e.sizes() == (5, 0, 0)


def test_from_functions_reproduces_the_analytic_targets_on_its_points():
    from oracle import solver as osol
    TP = pkg("data.tabulated").TabulatedProblem
    g = torch.Generator().manual_seed(5)
    p = TP.from_functions(osol.analytic_u, osol.analytic_u, osol.analytic_r, 40, 20, 30, generator=g, c_u=0.25)
    assert p.sizes() == (40, 20, 30) and p.c_u == 0.25 and p.coeffs == (1.0, 1.0, 1.0, 0.01, 0.01)
    assert torch.equal(p.u_ic, osol.analytic_u(p.X_ic)[:, 0]) and torch.equal(p.u_bc, osol.analytic_u(p.X_bc)[:, 0])
    assert torch.equal(p.r, osol.analytic_r(p.X_res)[:, 0])
    # the trainer's boxes: t = 0 face, x = 0 face, unit cube
    assert (p.X_ic[:, 0] == 0).all() and (p.X_bc[:, 1] == 0).all()
    for X in (p.X_res, p.X_ic, p.X_bc):
        assert (X >= 0).all() and (X < 1).all()
    assert p.X_res.std(0).min() > 0.2 and p.X_ic[:, 1:].std(0).min() > 0.2
    assert TP.from_functions(osol.analytic_u, osol.analytic_u, osol.analytic_r, 4, 0, 0).sizes() == (4, 0, 0)


# ---- 3. index draw
def test_dataset_indices():
    seed, step = 0x1234567887654321, 9
    for seg in range(3):
        for N in (1, 7, 1000, 2 ** 31 - 1):
            k = T.dataset_indices(seg, 0, 300, N, seed, step)
            assert k.dtype == np.int64 and k.min() >= 0 and k.max() < N
        assert not T.dataset_indices(seg, 0, 300, 1, seed, step).any()
        whole = T.dataset_indices(seg, 11, 130, 1000, seed, step)
        parts = [T.dataset_indices(seg, 11, 70, 1000, seed, step), T.dataset_indices(seg, 81, 60, 1000, seed, step)]
        assert np.array_equal(np.concatenate(parts), whole)
        assert set(T.dataset_indices(seg, 0, 4096, 16, seed, step)) == set(range(16))
    # the segments, steps and seeds draw different rows; a global index past 2^32 is its own counter
    a = T.dataset_indices(0, 0, 64, 1000, seed, step)
    for other in (T.dataset_indices(1, 0, 64, 1000, seed, step), T.dataset_indices(0, 0, 64, 1000, seed, step + 1),
                  T.dataset_indices(0, 0, 64, 1000, seed + 1, step), T.dataset_indices(0, 2 ** 32, 64, 1000, seed, step)):
        assert (a != other).mean() > 0.9
    # word 0 of the coordinate draw is the word behind the index: t = (word >> 8) 2^-24, idx = (word * N) >> 32
    import philox_reference as PR
    t = PR.draw(0, 0, 64, seed, step)[:, 0].astype(np.float64)
    assert np.abs(np.floor(t * 1000) - a).max() <= 1


# ---- 4. float64 step reference with targets
def test_reference_with_analytic_targets_is_the_analytic_reference():
    from oracle import solver as osol
    n, n_theta = 4, 12
    flat, X_ic, X_bc, X_res = step_inputs(50, n, n_theta, 9, 4, 5, salt=4)
    Xs = [x.double() for x in (X_ic, X_bc, X_res)]
    tg = [osol.analytic_u(Xs[0])[:, 0].numpy(), osol.analytic_u(Xs[1])[:, 0].numpy(), osol.analytic_r(Xs[2])[:, 0].numpy()]
    args = (flat, 50, n, n_theta, (1, 12), "cascade", haar_for(n, 1))
    g0, p0 = reference_loss(*args, *Xs)
    g1, p1 = T.reference_loss_data(*args, *Xs, *tg)
    assert np.abs(g1 - g0).max() < 1e-12 * max(1.0, np.abs(g0).max()) and np.abs(p1 - p0).max() < 1e-12
    # c_u is live: the zeroth-order term changes loss and gradient
    g2, p2 = T.reference_loss_data(*args, *Xs, *tg, c_u=0.7)
    assert abs(p2[0] - p0[0]) > 1e-3 and np.abs(g2 - g0).max() > 1e-3


def _blocks(n, n_theta):
    lay = pkg("hip.engine").param_layout(T.H, n, n_theta)
    o_post, o_th, NP = lay["postprocessor.0.weight"][0], lay["quantum_layer.params"][0], lay["__total__"][0]
    return {"pre": slice(0, o_post), "theta": slice(o_th, NP), "post": slice(o_post, o_th)}


@pytest.mark.parametrize("case,variant", [(c, v) for c, vs in T.CONTROLS.items() for v in vs])
def test_negative_controls_of_the_gpu_cases_are_not_vacuous(case, variant):
    """Each control must miss the true reference by more than 10 x the GPU tolerance, in a gradient block or a loss
    part: a GPU result within tolerance of the truth then fails the control with margin."""
    ans, n, L, *_ = T.CASES[case]
    n_theta = L * pkg("circuits").params_per_layer(ans, n)
    ref, bad = T.case_reference(case), T.case_reference(case, variant)
    worst = max(np.abs(ref["grad"][s] - bad["grad"][s]).max() / (TOL_G * max(1.0, np.abs(bad["grad"][s]).max()))
                for s in _blocks(n, n_theta).values())
    worst = max(worst, np.abs(ref["parts"] - bad["parts"]).max() / (TOL_L * max(1.0, np.abs(bad["parts"]).max())))
    assert worst > 10.0, worst
    assert np.abs(ref["grad"][_blocks(n, n_theta)["theta"]]).max() > 20 * TOL_G


# ---- 5. generic train(..., dataset=)
class Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(3, 8), nn.Tanh(), nn.Linear(8, 1))
        self.device, self.epochs = torch.device("cpu"), 2
        self.args = {"print_every": 10 ** 9, "solver": "Classical"}
        self.optimizer = torch.optim.Adam(self.parameters(), lr=1e-2)
        self.scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(self.optimizer)
        self.loss_fn, self.loss_history = nn.MSELoss(), []
        self.logger = type("Log", (), {"print": lambda self, *a: None})()

    def forward(self, x):
        return self.net(x)

    def save_state(self):
        pass


def test_generic_train_on_a_dataset_matches_a_hand_written_loop():
    trainer = pkg("trainer.diffusion_train")
    TP = pkg("data.tabulated").TabulatedProblem
    g = torch.Generator().manual_seed(3)
    co = dict(zip(("c_t", "c_x", "c_y", "d_xx", "d_yy"), T.COEFFS), c_u=T.C_U)
    ds = TP.from_functions(lambda X: torch.from_numpy(T.u_star(X)), lambda X: torch.from_numpy(T.u_star(X)),
                           lambda X: torch.from_numpy(T.r_star(X)), 50, 20, 30, generator=g, **co)
    torch.manual_seed(0)
    m = Tiny()
    ref = Tiny()
    ref.load_state_dict(m.state_dict())
    torch.manual_seed(11)
    trainer.train(m, batch_size=12, dataset=ds)
    assert len(m.loss_history) == 3
    # the same three steps by hand: randint rows IC -> BC -> residual, the residual with c_u u, 2 / 4 / 2 weights
    torch.manual_seed(11)
    c_t, c_x, c_y, d_xx, d_yy = T.COEFFS
    grad = lambda out, wrt: torch.autograd.grad(out, wrt, torch.ones_like(out), create_graph=True)[0]
    want = []
    for _ in range(3):
        ref.optimizer.zero_grad()
        ki, kb, kr = torch.randint(0, 20, (4,)), torch.randint(0, 30, (4,)), torch.randint(0, 50, (12,))
        t, x, y = (ds.X_res[kr][:, k:k + 1].clone().requires_grad_(True) for k in range(3))
        u = ref(torch.cat((t, x, y), 1))
        u_x, u_y = grad(u, x), grad(u, y)
        res = T.C_U * u + c_t * grad(u, t) + c_x * u_x + c_y * u_y - (d_xx * grad(u_x, x) + d_yy * grad(u_y, y))
        loss = 2.0 * ((res[:, 0] - ds.r[kr]) ** 2).mean() + 4.0 * ((ref(ds.X_bc[kb])[:, 0] - ds.u_bc[kb]) ** 2).mean() + \
            2.0 * ((ref(ds.X_ic[ki])[:, 0] - ds.u_ic[ki]) ** 2).mean()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm=1)
        ref.optimizer.step()
        ref.scheduler.step(loss)
        want.append(loss.item())
    assert np.allclose(m.loss_history, want, rtol=1e-6, atol=1e-7), (m.loss_history, want)
    # c_u is part of the trained residual
    ds0 = TP(ds.X_res, ds.r, ds.X_ic, ds.u_ic, ds.X_bc, ds.u_bc, **dict(co, c_u=0.0))
    torch.manual_seed(0)
    m0 = Tiny()
    torch.manual_seed(11)
    trainer.train(m0, batch_size=12, dataset=ds0)
    assert abs(m0.loss_history[0] - m.loss_history[0]) > 1e-3


def test_generic_train_refuses_an_empty_segment_behind_a_non_empty_batch():
    trainer = pkg("trainer.diffusion_train")
    TP = pkg("data.tabulated").TabulatedProblem
    (Xr, Xi, Xb), (r, ui, ub) = _segments()
    with pytest.raises(ValueError, match="boundary segment is empty"):
        trainer.train(Tiny(), batch_size=12, dataset=TP(Xr, r, Xi, ui, Xb[:0], ub[:0]))
