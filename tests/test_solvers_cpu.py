"""Solver tables of the multistep v-sampler on the host: ``syncfusion_amd.solvers.solver_table`` against the independent restatement
(tests/solver_ref.py), the first-order loop against the oracle sampler, one ``ab2`` step against the ODE solution of a manufactured
problem, and the convergence order of every solver on a Gaussian mixture with its exact denoiser."""
import functools
import math

import numpy as np
import pytest
import torch

import solver_ref
from oracle import sampler_ref

SOLVERS = ("ddim", "ab2", "dpmpp_2m")


def _schedules(T):
    from syncfusion_amd.diffusion import LinearSchedule, PowerSchedule

    return {"linear_1_0": LinearSchedule(1.0, 0.0)(T + 1), "linear_0.6_0.1": LinearSchedule(0.6, 0.1)(T + 1), "power_2": PowerSchedule(rho=2.0)(T + 1)}


@pytest.mark.parametrize("T", [1, 2, 3, 7, 150])
@pytest.mark.parametrize("name", ["linear_1_0", "linear_0.6_0.1", "power_2"])
def test_solver_table_matches_restatement(name, T):
    from syncfusion_amd.solvers import solver_table

    sig = _schedules(T)[name].numpy()
    assert sig.dtype == np.float32 and sig.shape == (T + 1,)
    first = solver_table(sig, "ddim")
    for solver in SOLVERS:
        got = solver_table(sig, solver)
        assert got.shape == (T, 5) and got.dtype == np.float64 and np.all(np.isfinite(got))
        worst = float(np.abs(got - solver_ref.table(sig, solver)).max())
        assert worst <= 1e-12, f"{solver}: largest difference {worst:.3e}"
        assert float(np.abs(got[:, 3] + got[:, 4] - first[:, 3]).max()) <= 1e-12, "c_0 + c_1 must be the first-order c_0"
        assert np.array_equal(got[:, :3], first[:, :3])
        assert got[0, 4] == 0.0 and np.array_equal(got[0], first[0])
    if T >= 2:
        assert np.any(solver_table(sig, "ab2")[1:, 4] != 0.0)
        # a dpmpp_2m row is second order only between finite lambdas: 1 -> 0 schedules lose a row at each end
        assert np.any(solver_table(sig, "dpmpp_2m")[:, 4] != 0.0) == (T >= 4 or name == "linear_0.6_0.1")


def test_power_schedule_values():
    from syncfusion_amd.diffusion import PowerSchedule

    s = PowerSchedule(0.9, 0.1, rho=3.0)(6).double().numpy()
    want = 0.1 + 0.8 * (1.0 - np.arange(6) / 5.0) ** 3.0
    assert np.abs(s - want).max() < 1e-7 and s[0] == np.float32(0.9) and s[-1] == np.float32(0.1)
    lin = PowerSchedule(rho=1.0)(11).numpy()
    assert np.abs(lin - np.linspace(1.0, 0.0, 11)).max() < 1e-7


def test_first_order_loop_is_the_oracle_sampler():
    g = torch.Generator().manual_seed(3)
    w = torch.randn(16, 16, generator=g) * 0.2

    def net(x, sig):
        return torch.tanh(x @ w) * (0.5 + sig[:, None]) - 0.3 * x

    x0 = torch.randn(4, 16, generator=g)
    for T in (1, 2, 9):
        want = sampler_ref.vsample(net, x0, T)
        got = solver_ref.multistep_sample(net, x0, sampler_ref.linear_schedule(T).numpy(), "ddim")
        assert float((got - want.double()).abs().max()) < 1e-6


# one ab2 step against the ODE, x0_hat(s) = A + B s exactly:  dx/dt = v = (cos t * x - (A + B t)) / sin t.  The solution carries a
# sin t * ln sin t term, so towards t = 0 it is integrated in tau = sqrt(t), where the right-hand side stays bounded and tends to 0.
@pytest.mark.parametrize("sigmas", [(0.8, 0.5, 0.35), (1.0, 0.7, 0.5), (0.3, 0.1, 0.0)], ids=["uneven", "from_pi_half", "to_zero"])
def test_ab2_step_is_exact_for_linear_x0(sigmas):
    from scipy.integrate import solve_ivp
    from syncfusion_amd.solvers import solver_table

    A, Bc, x_i = 0.7, -1.3, 0.45
    sig = np.asarray(sigmas, dtype=np.float32)
    t_p, t_i, t_n = (float(s) * math.pi / 2.0 for s in sig.astype(np.float64))
    al, be, cx, c0, c1 = solver_table(sig, "ab2")[1]
    assert abs(al - math.cos(t_i)) < 1e-15 and abs(be - math.sin(t_i)) < 1e-15
    step = cx * x_i + c0 * (A + Bc * t_i) + c1 * (A + Bc * t_p)

    def rhs(tau, x):
        t = tau * tau
        if t == 0.0:
            return [0.0]
        return [2.0 * tau * (math.cos(t) * x[0] - (A + Bc * t)) / math.sin(t)]

    sol = solve_ivp(rhs, (math.sqrt(t_i), math.sqrt(t_n)), [x_i], method="DOP853", rtol=1e-12, atol=1e-14)
    assert sol.success
    err = abs(step - float(sol.y[0, -1]))
    print(f"ab2 step vs solve_ivp {sigmas}: {err:.3e}")
    assert err < 1e-9
    if t_n == 0.0:
        assert abs(step - A) < 1e-12, "at t = 0 the sample is x0_hat(0)"


# convergence order on 0.5 N(-0.5, 0.3^2) + 0.5 N(0.6, 0.5^2) with the exact denoiser
MIX = ((0.5, -0.5, 0.3), (0.5, 0.6, 0.5))


def _x0_hat(x, t):
    a, b = math.cos(t), math.sin(t)
    logw, means = [], []
    for w, mu, s in MIX:
        var = a * a * s * s + b * b
        logw.append(math.log(w) - 0.5 * math.log(var) - 0.5 * (x - a * mu) ** 2 / var)
        means.append(mu + a * s * s / var * (x - a * mu))
    logw = np.stack(logw)
    r = np.exp(logw - logw.max(axis=0))
    r /= r.sum(axis=0)
    return (r * np.stack(means)).sum(axis=0)


@functools.lru_cache(maxsize=None)
def _solve(solver, T):
    from syncfusion_amd.solvers import solver_table

    sig = torch.linspace(1.0, 0.0, T + 1, dtype=torch.float32).numpy()
    tab = solver_table(sig, solver)
    t = sig.astype(np.float64) * (math.pi / 2.0)
    x = np.random.default_rng(0).standard_normal(1000)
    prev = np.zeros_like(x)
    for i in range(T):
        X = _x0_hat(x, t[i])            # = alpha x - beta v of the exact denoiser
        x = tab[i, 2] * x + tab[i, 3] * X + tab[i, 4] * prev
        prev = X
    return x


def _rms(solver, T):
    return float(np.sqrt(np.mean((_solve(solver, T) - _solve("ab2", 32768)) ** 2)))


def test_convergence_order():
    ratio = {s: _rms(s, 256) / _rms(s, 512) for s in SOLVERS}
    print("RMS error ratio T = 256 -> 512:", {k: round(v, 3) for k, v in ratio.items()})
    assert 1.9 <= ratio["ddim"] <= 2.1
    assert ratio["ab2"] >= 3.0
    assert ratio["dpmpp_2m"] >= 2.8


def test_ab2_beats_first_order_at_50_steps():
    e1, e2 = _rms("ddim", 50), _rms("ab2", 50)
    print(f"T = 50: ddim {e1:.3e}, ab2 {e2:.3e}")
    assert e2 < e1


def test_bad_sigmas_raise():
    from syncfusion_amd.solvers import check_sigmas, solver_table

    good = np.linspace(1.0, 0.0, 6, dtype=np.float32)
    assert solver_table(good, "ab2").shape == (5, 5)
    with pytest.raises(ValueError):
        check_sigmas(good, num_steps=6)                 # wrong length
    with pytest.raises(ValueError):
        solver_table(good[:1], "ab2")
    with pytest.raises(ValueError):
        solver_table(np.array([1.0, 0.5, 0.5, 0.0], dtype=np.float32), "ab2")      # not strictly decreasing
    with pytest.raises(ValueError):
        solver_table(good[::-1].copy(), "ab2")
    with pytest.raises(ValueError):
        solver_table(np.array([1.5, 0.5, 0.0], dtype=np.float32), "ddim")           # outside [0, 1]
    with pytest.raises(ValueError):
        solver_table(np.array([0.5, 0.2, -0.1], dtype=np.float32), "ddim")
    with pytest.raises(ValueError):
        solver_table(np.array([1.0, float("nan"), 0.0], dtype=np.float32), "ab2")
    with pytest.raises(ValueError):
        solver_table(good, "heun")


def test_diffusion_model_routes_sampler_solver():
    from helpers import SMALL_UNET
    from syncfusion_amd.diffusion import DiffusionModel, PowerSchedule, UNetV0, VDiffusion, VSampler

    def build(**kw):
        return DiffusionModel(net_t=functools.partial(UNetV0, seed=1), diffusion_t=VDiffusion, sampler_t=VSampler, use_embedding_cfg=True, **SMALL_UNET, **kw)

    assert build().sampler.solver == "ddim"
    m = build(sampler_solver="ab2", sampler_schedule=PowerSchedule(rho=3.0))
    assert m.sampler.solver == "ab2" and m.sampler.schedule.rho == 3.0
    assert not any(k.startswith("sampler") for k in m.state_dict()), "the sampler adds nothing to the checkpoint layout"
    with pytest.raises(ValueError):
        build(sampler_solver="heun")


def test_exports():
    import syncfusion_amd as sa

    assert sa.solver_table is __import__("syncfusion_amd.solvers", fromlist=["solver_table"]).solver_table
    assert all(n in sa.__all__ for n in ("solver_table", "PowerSchedule", "vary_batch"))
