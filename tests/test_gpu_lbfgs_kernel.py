"""``qc_lbfgs_step`` on synthetic flat vectors, as tests/test_gpu_optim.py drives ``qc_adam_step``: every call is compared with
the float64 restatement of the header's rule (tests/lbfgs_reference.py) fed the same values, FIXED mode with torch.optim.LBFGS
as well.

Parameter tolerance.  Not fixed in advance: the reference runs once in float32 and once in float64 on the same sequence, on the
CPU, inside the test; the kernel is allowed 4 x their gap (largest entry) at every call.  The margin is there because the
kernel's reduction order and its Gram form of the recursion differ from the reference's fp32 order.  The step length t gets
the same 4 x gap plus 8 x 2^-24 t: t is lr (exact), a product with a shrink factor (one rounding) or the quotient t_q of
quantities that each carry a few roundings, so two fp32 evaluations can agree by luck where a third differs by a few ulp.
Measured on an MI355X (largest gap over the calls of a case; the kernel's largest error / gap over the calls):
  FIXED, quartic, lr 0.2:  NP 5: gaps 4.6e-8 .. 4.5e-7, kernel at 1.0 .. 3.4 x     NP 717: 4.3e-7 .. 2.2e-6, 1.0 x
                           NP 3069 / 3070 / 4000: 4.6e-7 .. 2.3e-6, 1.0 .. 1.3 x
  ARMIJO, scripted:        NP 5: 5.3e-7 (m 1), 6.1e-4 (m 3), 1.7e-2 (m 10), 3.6e-2 (m 32), kernel at 0.8 .. 1.5 x
                           NP 717: 3.1e-7 .. 1.9e-5, 1.0 .. 1.1 x     NP 3069 / 3070 / 4000: 3.5e-7 .. 2.1e-5, 1.0 .. 1.1 x
  every branch (m 3):      NP 717: 4.4e-6, 1.0 x     NP 4000: 9.3e-6, 1.0 x
(The first form of the kernel, fp32 scalars throughout, missed the bound at FIXED NP 5, m 10: 5.7e-7 against 4 x 1.43e-7.)
Conditions on the inputs, asserted below on the references (CPU arithmetic only):
  * at every ARMIJO trial |f - (f0 + c1 t gtd0)| >= 1e-3 max(1, |f0|), so fp32 rounding cannot flip a decision;
  * the scripted sequences are well-posed for a bound of "4 x one float32 run": the rule with float32 vectors and float64 dot
    products (tests/lbfgs_reference.py, acc=float64: the most an implementation with fp32 vectors can do) stays within 2 x
    the gap at every call.  The gap of ONE float32 run is a noisy measure at NP = 5, where two roundings in five entries decide
    it: on 4 of the first 16 seeds of NP = 5, m = 3 that more precise CPU run itself ends 4.0 .. 4.9 gaps from float64.  The
    seeds are the first ones that meet both conditions (round 0 for 18 of the 20 shapes, 1 for (5, 3), 2 for (5, 10))."""
import numpy as np
import pytest
import torch

import lbfgs_driver as D
import lbfgs_reference as LR
from conftest import pkg

pytestmark = pytest.mark.gpu

SHAPES = [(NP, m) for NP in (5, 717, 3069, 3070, 4000) for m in (1, 3, 10, 32)]
SEED_ROUND = {(5, 3): 1, (5, 10): 2}        # see the module docstring; every other shape takes round 0
COUNTERS = ("n_eval", "n_iter", "n_pairs", "ls_trials", "n_rejected", "n_skipped_pairs", "n_resets", "stalled", "accepted")


def _check_params(tag, k, got, pair, gap, worst):
    err = float(np.abs(got.astype(np.float64) - pair.x64).max())
    worst.append((err, gap))
    assert np.isfinite(got).all(), (tag, k)
    assert err <= 4.0 * gap, (tag, k, err, gap)


@pytest.mark.parametrize("NP,m", SHAPES)
def test_fixed_mode_matches_reference_and_torch(NP, m, gpu_device):
    """2 m + 3 evaluations of a convex quartic, evaluated on the host in float64 at the device's own parameters (the ring
    wraps), lr = 0.2: parameters after every call against the float64 reference and against torch.optim.LBFGS(lr,
    max_iter=1, history_size=m, tolerance_grad=0, tolerance_change=0, line_search_fn=None) fed the same values."""
    fg = LR.quartic(NP, seed=NP + m)
    x0 = (0.5 * np.random.default_rng(NP * 7 + m).standard_normal(NP)).astype(np.float32)
    dev = D.Device(NP, x0, gpu_device, m, "fixed", lr=0.2)
    pair = D.RefPair(NP, x0, m, "fixed", lr=0.2)
    pt = torch.nn.Parameter(torch.from_numpy(x0.astype(np.float64)))
    opt = torch.optim.LBFGS([pt], lr=0.2, max_iter=1, history_size=m, tolerance_grad=0, tolerance_change=0, line_search_fn=None)
    fed = {}

    def closure():
        pt.grad = torch.from_numpy(fed["g"].astype(np.float64))
        return torch.tensor(fed["f"])

    worst, x = [], x0
    for k in range(2 * m + 3):
        f, g = fg(x)
        parts, g32 = D.parts_of(f), g.astype(np.float32)
        fed["f"], fed["g"] = D.f_of(parts), g32
        gap = pair.step(parts, g32)
        opt.step(closure)
        x = dev.call(parts, g32)
        dev.assert_guards()
        _check_params("fixed", k, x, pair, gap, worst)
        assert float(np.abs(x.astype(np.float64) - pt.detach().numpy()).max()) <= 4.0 * gap + 1e-12, k
        assert np.abs(pair.x64 - pt.detach().numpy()).max() < 1e-9
    rec = dev.st.read()
    assert rec["n_eval"] == 2 * m + 3 == rec["n_iter"] and rec["n_pairs"] == pair.r64.n_pairs == m
    print("fixed NP %d m %d: worst err / gap = %.2f, largest gap %.2e" % (NP, m, max(e / g for e, g in worst if g > 0),
                                                                          max(g for _, g in worst)))


def _run_script(NP, m, script, seed, gpu_device, max_ls=10, device_only=False):
    """Feed a scripted sequence to the device and the reference pair; after every call the accept flag, t, the counters
    and the parameters.  Returns the per-call parameters of the device (bit patterns) and the final record."""
    seq, _ = D.scripted(NP, m, script, seed, max_ls=max_ls)
    x0 = np.random.default_rng(seed + 1).standard_normal(NP).astype(np.float32)
    dev = D.Device(NP, x0, gpu_device, m, "armijo", max_ls=max_ls)
    pair = D.RefPair(NP, x0, m, "armijo", mixed=True, max_ls=max_ls)
    worst, bits, k = [], [], 0
    for ev in seq:
        if ev[0] == "restart":
            dev.st.restart(ev[1])
            pair.restart(ev[1])
            continue
        _, parts, g = ev
        x = dev.call(parts, g)
        bits.append(x.view(np.int32).copy())
        if not device_only:
            gap = pair.step(parts, g)
            r64, r32 = pair.r64, pair.r32
            assert D.slack_ok(r64), (k, r64.slack, r64.slack_f0)            # the condition on the inputs
            assert r32.counters() == r64.counters(), k                       # (fp32 itself takes the same branches)
            assert pair.mixed_err <= 2.0 * gap, (k, pair.mixed_err, gap)     # the sequence is well-posed for the bound
            dev.assert_guards()
            rec = dev.st.read()
            assert {c: rec[c] for c in COUNTERS} == r64.counters(), (k, script[:k + 2], rec, r64.counters())
            t64 = float(r64.t)
            assert abs(rec["t"] - t64) <= 4.0 * abs(float(r32.t) - t64) + 8 * 2.0 ** -24 * abs(t64), (k, rec["t"], t64)
            assert abs(rec["t_led"] - float(r64.t_led)) <= 4.0 * abs(float(r32.t_led) - float(r64.t_led)) + 8 * 2.0 ** -24 * abs(t64)
            _check_params(script, k, x, pair, gap, worst)
        k += 1
    if not device_only:
        rows = dev.st.history()
        want = np.array([(r[0], r[1], r[2]) for r in pair.r64.rows])
        assert rows.shape == want.shape
        assert np.array_equal(rows[:, 2], want[:, 2])
        fin = np.isfinite(want[:, 0])
        assert np.allclose(rows[fin, 0], want[fin, 0], rtol=1e-6, atol=0) and np.isnan(rows[~fin, 0]).all()
        print("armijo NP %d m %d %s...: worst err / gap = %.2f, largest gap %.2e"
              % (NP, m, script[:12], max(e / g for e, g in worst if g > 0), max(g for _, g in worst)))
    return bits, dev.st.read(), pair, dev


@pytest.mark.parametrize("NP,m", SHAPES)
def test_armijo_mode_matches_reference(NP, m, gpu_device):
    """2 m + 3 evaluations, accepted points with interpolated and clamped rejections in between; the ring wraps."""
    script = "F" + "".join("AAQAACA"[i % 7] for i in range(2 * m + 2))
    _, rec, pair, _ = _run_script(NP, m, script, NP * 100 + m + 1000 * SEED_ROUND.get((NP, m), 0), gpu_device)
    assert rec["n_pairs"] == m and rec["n_iter"] > m + 1 and rec["n_rejected"] >= 1


# every branch of the backtracking mode, max_ls = 3: interpolated and clamped rejections, a NaN loss, an inf gradient entry,
# a skipped pair, the non-descent reset (g = 0), an exhausted search and the steepest-descent restart behind it, an accepted
# point after that, two exhausted searches in a row ending in stalled, two calls while stalled, then restarts without and
# with the history
BRANCHES = "FAAQACANAIASAZAAA" + "NNN" + "AAA" + "NNN" + "NNN" + "QA" + "RFAAQA" + "KFAA"


@pytest.mark.parametrize("NP", [717, 4000])
def test_armijo_every_branch(NP, gpu_device):
    _, rec, pair, _ = _run_script(NP, 3, BRANCHES, 40 + NP, gpu_device, max_ls=3)
    r = pair.r64
    acc = [row[2] for row in r.rows]
    i = BRANCHES.index("NNNNNN")                          # (letters and evaluations coincide up to the first restart)
    assert acc[i:i + 8] == [0] * 8                        # two exhausted searches, then the two calls while stalled
    assert r.n_skipped_pairs == 2 and r.n_resets == 3     # S and the A behind Z (s = 0); Z and two exhausted searches (the third stalls)
    assert rec["stalled"] == 0 and rec["n_pairs"] == r.n_pairs == 3          # K kept the three pairs of the R segment


@pytest.mark.parametrize("NP", [717, 4000])
def test_two_runs_are_bit_identical(NP, gpu_device):
    a, rec_a, _, dev_a = _run_script(NP, 3, BRANCHES, 40 + NP, gpu_device, max_ls=3, device_only=True)
    b, rec_b, _, dev_b = _run_script(NP, 3, BRANCHES, 40 + NP, gpu_device, max_ls=3, device_only=True)
    assert len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))
    assert rec_a == rec_b
    assert torch.equal(dev_a.st.ws.view(torch.int32), dev_b.st.ws.view(torch.int32))
    assert torch.equal(dev_a.st.hist.view(torch.int32), dev_b.st.hist.view(torch.int32))


@pytest.mark.parametrize("NP", [300, 3200])
def test_tables_follow_the_new_theta(NP, gpu_device):
    """A cascade n = 4 program whose parameters are the last entries of the vector: after a call the trig table and the
    diagonal-run tables equal qc_prepare_gates on the new theta (register path and strided path)."""
    circuits, engine = pkg("circuits"), pkg("hip.engine")
    prog = circuits.build_program("cascade", 4, 2, True)
    haar = circuits.haar_unitaries(3, 4)
    circ, fresh = engine.Circuit(prog, haar, gpu_device), engine.Circuit(prog, haar, gpu_device)
    theta_off = NP - prog.n_params
    seq, _ = D.scripted(NP, 3, "FAQA", 9)
    x0 = np.random.default_rng(10).standard_normal(NP).astype(np.float32)
    dev = D.Device(NP, x0, gpu_device, 3, "armijo", circuit=circ, theta_off=theta_off)
    for _, parts, g in seq:
        x = dev.call(parts, g)
        fresh.prepare(dev.prm[theta_off:NP].clone())
        assert torch.equal(circ.trig.view(torch.int32), fresh.trig.view(torch.int32))
    assert float(np.abs(x - x0).max()) > 1e-3
