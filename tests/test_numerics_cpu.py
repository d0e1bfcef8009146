"""The numerics regimes of tests/numerics.py tell a one-pass variance from a shifted one (CPU only, no GPU).

An fp32 emulation of the chunked GroupNorm statistics -- per-thread partials, a serial merge, Chan across chunks -- in the one-pass
form (M2 = sum x^2 - sum x * mean of raw values) must FAIL the gates the GPU tests apply at the offset and dead-channel regimes, and
the pivot-shifted form must pass them: otherwise the GPU tests could not see the difference either.  Also: check_close catches a
defect confined to one group that the whole-tensor rel-L2 lets through, and names where it is.
"""
import pytest
import torch

import numerics as nx

GN_TOL = 2e-6          # test_gpu_ops.py: the fp32 GroupNorm+SiLU gate
B, L, C, G, CHUNK = 1, 704, 16, 2, 176   # 5632-element groups in four 1408-element chunks (256 per-thread partials each)


def _normalised(x, shifted):
    mean, var = nx.chunk_stats_fp32(x, G, CHUNK, shifted)
    cpg = C // G
    m = mean.float().repeat_interleave(cpg, dim=1)[:, None, :]
    rstd = torch.rsqrt(var.float() + 1e-5).repeat_interleave(cpg, dim=1)[:, None, :]
    return (x - m) * rstd                                  # fp32 arithmetic, as the kernels apply it


def _regime_case(regime, seed=0):
    x = nx.grouped_input(B, L, C, G, regime, torch.Generator().manual_seed(seed))
    ref = nx.group_norm_cl64(x, G, torch.ones(C), torch.zeros(C), 1e-5)
    return x, ref


def _gate(regime):
    kind, _, val = regime.partition(":")
    ratio = float(val) if kind == "offset" else 1e3   # dead channels: sigma = 1e-3 |mu|
    return nx.offset_gate(GN_TOL, ratio)


@pytest.mark.parametrize("regime", ["offset:30", "offset:300", "dead:1", "dead:4"])
def test_one_pass_statistics_fail_the_offset_gates(regime):
    x, ref = _regime_case(regime)
    assert nx.group_ratio(x, G) > 20
    with pytest.raises(AssertionError):
        nx.check_close(_normalised(x, shifted=False), ref, _gate(regime), f"one-pass {regime}")


@pytest.mark.parametrize("regime", ["offset:3", "offset:30", "offset:300", "dead:1", "dead:4"])
def test_shifted_statistics_pass_the_offset_gates(regime):
    x, ref = _regime_case(regime)
    nx.check_close(_normalised(x, shifted=True), ref, _gate(regime), f"shifted {regime}")


def test_constant_groups_normalise_to_beta():
    """variance 0: (x - mean) must come out 0, not the rounding noise of the mean times 1 / sqrt(eps) (beta = 1 keeps the reference
    away from zero so that the relative gates mean something)"""
    x, ref = _regime_case("const")
    nx.check_close(_normalised(x, shifted=True) + 1.0, ref + 1.0, GN_TOL, "shifted const")


def test_low_offset_does_not_separate_the_forms():
    """mean/std = 3 (the suite's usual inputs are ~0.3): both forms pass -- which is why the suite needed the regimes above."""
    x, ref = _regime_case("offset:3")
    nx.check_close(_normalised(x, shifted=False), ref, _gate("offset:3"), "one-pass offset:3")


def test_regimes_reach_their_ratios():
    g = torch.Generator().manual_seed(1)
    for r in nx.OFFSET_RATIOS:
        x = nx.grouped_input(2, 256, 32, 4, f"offset:{r:g}", g)
        assert 0.7 * r < nx.group_ratio(x, 4) < 2.0 * r
    x = nx.grouped_input(2, 256, 32, 4, "dead:4", g)
    assert nx.group_ratio(x, 4) > 500
    x = nx.grouped_input(2, 256, 32, 4, "const", g)
    xg = x.reshape(2, 256, 4, 8)
    assert bool((xg == xg[:, :1, :, :1]).all())


def test_check_close_flags_one_bad_group_that_rel_l2_passes():
    g = torch.Generator().manual_seed(2)
    Bc, Lc, Cc, Gc = 4, 64, 128, 32
    ref = torch.randn(Bc, Lc, Cc, generator=g, dtype=torch.float64)
    got = ref.clone()
    cpg = Cc // Gc
    got[2, :, 5 * cpg:6 * cpg] *= 1 + 1.5e-4              # clip 2, group 5: off by 1.5e-4 relative
    tol = 2e-5
    rel = float((got - ref).norm() / ref.norm())
    assert rel < tol                                        # the whole-tensor rel-L2 alone lets it through
    with pytest.raises(AssertionError) as e:
        nx.check_close(got, ref, tol, "one bad group")
    msg = str(e.value)
    assert "clip 2" in msg and "max|err|" in msg
    ch = int(msg.split("channel ")[1].split(")")[0])
    assert 5 * cpg <= ch < 6 * cpg


def test_check_close_rejects_nan():
    ref = torch.ones(2, 3, 4)
    got = ref.clone()
    got[1, 2, 3] = float("nan")
    with pytest.raises(AssertionError, match=r"non-finite.*clip 1, row 2, channel 3"):
        nx.check_close(got, ref, 1e-3, "nan")


def test_peaked_scores_have_the_requested_spread_and_peak():
    g = torch.Generator().manual_seed(3)
    Bq, Lq, H, D = 2, 100, 2, 64
    for s in nx.PEAK_STDS:
        for where, j in (("first", 0), ("middle", 50), ("last", 99)):
            q, k = nx.peaked_qk(Bq, Lq, H, D, s, where, g)
            qs = q.double().reshape(Bq, Lq, H, D).transpose(1, 2)
            ks = k.double().reshape(Bq, Lq, H, D).transpose(1, 2)
            sim = qs @ ks.transpose(-1, -2) * D ** -0.5
            others = torch.cat([sim[..., :j], sim[..., j + 1:]], dim=-1)
            assert 0.6 * s < float(others.std()) < 1.6 * s
            assert bool((sim.argmax(-1) == j).float().mean() > 0.9)          # the dominant key wins for (almost) every query
