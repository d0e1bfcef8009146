"""Guidance schedules on the host: syncfusion_amd.guidance (scale_table, plan_segments, evaluation_rows) and the properties of the fp64
restatement (tests/guidance_ref.py) the GPU tests compare against."""
import numpy as np
import pytest
import torch

import guidance_ref
from syncfusion_amd.guidance import check_rescale, evaluation_rows, plan_segments, scale_table

T, B = 6, 3
SIG = np.linspace(1.0, 0.0, T + 1, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# scale_table
# ---------------------------------------------------------------------------------------------------------------------------------
def test_scale_table_accepts_every_form():
    t = scale_table(2.5, SIG, B)
    assert t.shape == (T, B) and t.dtype == np.float32 and np.all(t == 2.5)
    assert np.all(scale_table(np.float32(2.5), SIG, B) == 2.5) and np.all(scale_table(3, SIG, B) == 3.0)
    per_clip = np.array([1.0, 3.0, 7.5])
    for form in (per_clip, list(per_clip), torch.tensor(per_clip), torch.tensor(per_clip, dtype=torch.float32)):
        t = scale_table(form, SIG, B)
        assert t.shape == (T, B) and np.all(t == per_clip[None, :].astype(np.float32))
    per_step = np.linspace(1.0, 6.0, T)
    t = scale_table(per_step, SIG, B)
    assert np.all(t == per_step[:, None].astype(np.float32))
    full = np.arange(T * B, dtype=np.float64).reshape(T, B) / 4.0
    assert np.array_equal(scale_table(full, SIG, B), full.astype(np.float32))
    assert np.array_equal(scale_table(torch.tensor(full), SIG, B), full.astype(np.float32))
    # a 1-D array of length T == B is read per clip
    sq = scale_table(np.array([1.0, 2.0, 3.0]), SIG[:4], 3)
    assert np.all(sq == np.array([1.0, 2.0, 3.0], dtype=np.float32)[None, :])
    # the result is the caller's to change
    t = scale_table(per_clip, SIG, B)
    t[0, 0] = 9.0
    assert per_clip[0] == 1.0
    assert np.array_equal(scale_table(full, SIG, B), guidance_ref.scales(full, SIG, B).astype(np.float32))


def test_scale_table_interval():
    t = scale_table(4.0, SIG, B, guidance_interval=(0.3, 0.8))
    inside = (SIG[:T] >= 0.3) & (SIG[:T] <= 0.8)
    assert inside.tolist() == [False, False, True, True, True, False]
    assert np.all(t[inside] == 4.0) and np.all(t[~inside] == 1.0)
    assert np.array_equal(t, guidance_ref.scales(4.0, SIG, B, (0.3, 0.8)).astype(np.float32))
    # the ends are inside; the level of a step is sigmas[i], the level it evaluates the net at (the last sigma is never one)
    ends = scale_table(4.0, SIG, B, guidance_interval=(float(SIG[4]), float(SIG[2])))
    assert (ends[:, 0] != 1.0).tolist() == [False, False, True, True, True, False]
    assert np.all(scale_table(4.0, SIG, B, guidance_interval=(0.0, 0.0)) == 1.0)
    assert np.all(scale_table(4.0, SIG, B, guidance_interval=(0.5, 0.5))[:, 0] == np.where(SIG[:T] == 0.5, 4.0, 1.0))
    per = scale_table(np.array([1.0, 3.0, 7.5]), SIG, B, guidance_interval=[0.3, 0.8])
    assert np.all(per[~inside] == 1.0) and np.all(per[inside] == np.array([1.0, 3.0, 7.5], dtype=np.float32))


@pytest.mark.parametrize("bad", [np.nan, np.inf, [1.0, np.nan, 2.0], np.ones(4), np.ones((T, B + 1)), np.ones((B, T)), np.ones((T, B, 1)),
                                 np.ones(0), "7.5", None, True], ids=repr)
def test_scale_table_rejects(bad):
    with pytest.raises(ValueError):
        scale_table(bad, SIG, B)


def test_scale_table_rejects_bad_intervals_and_schedules():
    for iv in [(0.8, 0.3), (0.3,), (0.1, 0.2, 0.3), (np.nan, 0.5), (0.0, np.inf)]:
        with pytest.raises(ValueError):
            scale_table(2.0, SIG, B, guidance_interval=iv)
    with pytest.raises(ValueError):
        scale_table(2.0, SIG[::-1], B)
    with pytest.raises(ValueError):
        scale_table(2.0, SIG, 0)
    for phi in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            check_rescale(phi)
    assert check_rescale(0) == 0.0 and check_rescale(1) == 1.0 and check_rescale(np.float32(0.5)) == 0.5


# ---------------------------------------------------------------------------------------------------------------------------------
# plan_segments / evaluation_rows on hand-written tables
# ---------------------------------------------------------------------------------------------------------------------------------
def test_plan_all_ones():
    segs = plan_segments(np.ones((T, B), dtype=np.float32))
    assert segs == [(0, T, False)] and evaluation_rows(segs, B) == T * B


def test_plan_all_guided():
    segs = plan_segments(np.full((T, B), 7.5, dtype=np.float32))
    assert segs == [(0, T, True)] and evaluation_rows(segs, B) == 2 * T * B


def test_plan_interval_in_the_middle():
    t = np.ones((T, B), dtype=np.float32)
    t[2:5] = 3.0
    segs = plan_segments(t)
    assert segs == [(0, 2, False), (2, 5, True), (5, 6, False)]
    assert evaluation_rows(segs, B) == (2 + 1) * B + 3 * 2 * B
    assert plan_segments(scale_table(3.0, SIG, B, (0.3, 0.8))) == segs


def test_plan_one_clip_guided_throughout():
    t = np.ones((T, B), dtype=np.float32)
    t[:, 1] = 2.0
    segs = plan_segments(t)
    assert segs == [(0, T, True)] and evaluation_rows(segs, B) == 2 * T * B


def test_plan_alternating_and_degenerate():
    t = np.ones((5, 2), dtype=np.float32)
    t[0, 0] = t[2, 1] = t[4, 0] = 0.5                     # (a scale below 1 is guidance too)
    segs = plan_segments(t)
    assert segs == [(0, 1, True), (1, 2, False), (2, 3, True), (3, 4, False), (4, 5, True)]
    assert evaluation_rows(segs, 2) == 3 * 4 + 2 * 2
    assert plan_segments(np.ones((1, 1))) == [(0, 1, False)]
    with pytest.raises(ValueError):
        plan_segments(np.ones(4))
    with pytest.raises(ValueError):
        plan_segments(np.ones((0, 2)))
    for s in (plan_segments(t), plan_segments(np.ones((7, 3)))):
        assert s[0][0] == 0 and all(a[1] == b[0] and a[2] != b[2] for a, b in zip(s, s[1:]))


# ---------------------------------------------------------------------------------------------------------------------------------
# properties of the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def _vs(seed=3, shape=(3, 2, 515)):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64) + 0.3, 0.5 * torch.randn(shape, generator=g, dtype=torch.float64) - 0.1


def test_ref_phi_zero_is_plain_guidance():
    v_c, v_u = _vs()
    s = [2.0, 1.0, 7.5]
    out = guidance_ref.guided(v_c, v_u, s, 0.0)
    for b in range(3):
        assert torch.equal(out[b], v_c[b] if s[b] == 1.0 else v_u[b] + s[b] * (v_c[b] - v_u[b]))


def test_ref_phi_one_restores_the_level_of_v_c():
    v_c, v_u = _vs()
    out = guidance_ref.guided(v_c, v_u, [2.0, 4.0, 7.5], 1.0)
    for b in range(3):
        want, got = float(v_c[b].std(unbiased=False)), float(out[b].std(unbiased=False))
        assert abs(got - want) <= 1e-12 * want
        # the biased / unbiased choice cancels in the ratio
        assert abs(float(out[b].std(unbiased=True)) - float(v_c[b].std(unbiased=True))) <= 1e-12 * want
    half = guidance_ref.guided(v_c, v_u, [2.0, 4.0, 7.5], 0.5)
    plain = guidance_ref.guided(v_c, v_u, [2.0, 4.0, 7.5], 0.0)
    assert torch.allclose(half, 0.5 * (plain + out), rtol=1e-13, atol=0)
    # a constant guided direction (std 0) is left alone
    flat = torch.ones_like(v_c)
    assert torch.equal(guidance_ref.guided(flat, flat, [2.0, 2.0, 2.0], 1.0), flat)


def test_ref_scale_one_does_not_read_v_u():
    v_c, v_u = _vs()
    for phi in (0.0, 0.7):
        a = guidance_ref.guided(v_c, v_u, [1.0, 1.0, 1.0], phi)
        assert torch.equal(a, guidance_ref.guided(v_c, None, [1.0, 1.0, 1.0], phi)) and torch.equal(a, v_c)
        mixed = guidance_ref.guided(v_c, v_u, [1.0, 3.0, 1.0], phi)
        poisoned = v_u.clone()
        poisoned[0], poisoned[2] = float("nan"), float("inf")
        assert torch.equal(mixed, guidance_ref.guided(v_c, poisoned, [1.0, 3.0, 1.0], phi))
        assert torch.equal(mixed[0], v_c[0]) and torch.equal(mixed[2], v_c[2])


def test_ref_loop_asks_for_v_u_only_on_guided_steps():
    calls = {"c": 0, "u": 0}

    def net_c(x, s):
        calls["c"] += 1
        return 0.1 * x + s.reshape(-1, 1, 1)

    def net_u(x, s):
        calls["u"] += 1
        return -0.2 * x

    x0 = torch.randn(B, 1, 64, generator=torch.Generator().manual_seed(1))
    table = scale_table(3.0, SIG, B, (0.3, 0.8))
    out = guidance_ref.sample(net_c, net_u, x0, SIG, "ab2", table, phi=0.7)
    assert calls == {"c": T, "u": 3} and out.dtype == torch.float64 and bool(torch.isfinite(out).all())
    # all ones: solver_ref's loop
    import solver_ref

    ones = guidance_ref.sample(net_c, net_u, x0, SIG, "ab2", np.ones((T, B)), phi=0.7)
    assert torch.equal(ones, solver_ref.multistep_sample(net_c, x0, SIG, "ab2"))
    # a restart at a seam drops the history: another result with a second-order rule, the same with the first-order one
    assert not torch.equal(guidance_ref.sample(net_c, net_u, x0, SIG, "ab2", table, restart_at=(2, 5)), guidance_ref.sample(net_c, net_u, x0, SIG, "ab2", table))
    assert torch.equal(guidance_ref.sample(net_c, net_u, x0, SIG, "ddim", table, restart_at=(2, 5)), guidance_ref.sample(net_c, net_u, x0, SIG, "ddim", table))


# ---------------------------------------------------------------------------------------------------------------------------------
# public surface
# ---------------------------------------------------------------------------------------------------------------------------------
def test_diffusion_model_routes_the_guidance_keys():
    import functools

    from helpers import SMALL_UNET
    from syncfusion_amd.diffusion import DiffusionModel, UNetV0, VDiffusion, VSampler

    def build(**kw):
        return DiffusionModel(net_t=functools.partial(UNetV0, seed=1), diffusion_t=VDiffusion, sampler_t=VSampler, use_embedding_cfg=True, **SMALL_UNET, **kw)

    plain = build().sampler
    assert plain.guidance_rescale == 0.0 and plain.guidance_interval is None and plain.last_segments is None
    m = build(sampler_guidance_rescale=0.7, sampler_guidance_interval=[0.3, 0.8], sampler_solver="ab2")
    assert m.sampler.guidance_rescale == 0.7 and m.sampler.guidance_interval == (0.3, 0.8) and m.sampler.solver == "ab2"
    assert not any(k.startswith("sampler") for k in m.state_dict()), "the sampler adds nothing to the checkpoint layout"
    with pytest.raises(ValueError):
        build(sampler_guidance_rescale=1.5)


def test_exports_and_signatures():
    import inspect

    import syncfusion_amd as sa
    from syncfusion_amd import _lib

    for name in ("scale_table", "plan_segments", "evaluation_rows"):
        assert name in sa.__all__ and getattr(sa, name) is getattr(sa.guidance, name)
    for fn in (sa.generate_batch, sa.generate_dataset, sa.vary_batch, sa.VSampler.forward):
        params = inspect.signature(fn).parameters
        assert "guidance_rescale" in params and "guidance_interval" in params and "embedding_scale" in params, fn
    for sym in ("sf_vsample_gx", "sf_vsample_gx_workspace_bytes", "sf_op_guidance_stats", "sf_op_guidance_stats_bytes", "sf_op_vsampler_update_g"):
        assert sym in _lib.SYMBOLS
