"""The per-element gate of tests/onset_layers_ref.py is tested before it is trusted (CPU only, no GPU).

* The restated BatchNorm fold and the rounding helpers are pinned against direct fp64 computations.
* A CPU emulation of a CORRECT kernel (the same rounded operands, conv3d accumulated in fp32, one output rounding) passes the gate for
  every convolution geometry of the network, with and without a residual, cin from 3 to 512, in bf16, fp16 and fp32.
* Five planted faults of the kind a tiled kernel produces each FAIL the gate in every dtype, and each PASSES the stage-level
  whole-tensor rel-L2 gate (test_gpu_models.ONSET_TAP_TOL) at the size of the real tap -- which is why the gate exists.
"""
import math

import pytest
import torch

import onset_layers_ref as R
from test_gpu_models import ONSET_TAP_TOL

DTYPES = ["fp32", "bf16", "fp16"]
N32_ROWS = {"layer1": 32 * 30 * 56 * 56, "layer2": 32 * 30 * 28 * 28, "stem_odd": 32 * 30 * 57 * 56}   # rows of the benchmarked taps


# ---------------------------------------------------------------------------------------------------------------------------------
# the fold and the rounding helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def test_fold_bn_against_fp64():
    g = torch.Generator().manual_seed(0)
    c = 4096
    gam, b, m = torch.randn(c, generator=g), torch.randn(c, generator=g), 3 * torch.randn(c, generator=g)
    v = torch.exp(torch.rand(c, generator=g) * (math.log(1e2) - math.log(1e-3)) + math.log(1e-3))
    sc, shift = R.fold_bn(gam, b, m, v)
    assert sc.dtype == shift.dtype == torch.float32
    sc64 = gam.double() / torch.sqrt(v.double() + float(torch.tensor(R.BN_EPS, dtype=torch.float32)))
    # v + eps, sqrt and the divide are one correctly rounded fp32 operation each: three roundings, (1 + 2^-24)^3 - 1 < 2^-22
    assert bool(((sc.double() - sc64).abs() <= 2.0 ** -22 * sc64.abs()).all())
    sh64 = b.double() - m.double() * sc.double()
    assert bool(((shift.double() - sh64).abs() <= 2.0 ** -23 * (b.abs() + (m * sc).abs()).double()).all())   # product and difference
    # eps is the fp32 1e-5f; and sc is the correctly rounded quotient: no fp32 value is nearer to g / sqrt(eps)
    sc0 = R.fold_bn(gam, b, m, torch.zeros(c))[0]
    q = gam.double() / torch.sqrt(torch.tensor(1e-5, dtype=torch.float32).double()).float().double()
    for nb in (torch.nextafter(sc0, torch.full_like(sc0, float("inf"))), torch.nextafter(sc0, torch.full_like(sc0, -float("inf")))):
        assert bool(((sc0.double() - q).abs() <= (nb.double() - q).abs()).all())


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_rounding_helpers(dtype):
    u = R.U[dtype]
    x = torch.randn(1 << 16, generator=torch.Generator().manual_seed(1)) * 3
    r = R.round_to(x, dtype)
    assert bool(((r - x).abs().double() <= u * x.abs().double()).all()) and float(((r - x).abs() / x.abs()).max()) > 0.9 * u
    assert torch.equal(R.round_once(x.double(), dtype), r.double())          # one rounding of an fp32 value either way
    # ties go to even, in both helpers
    one = torch.tensor([1.0 + u, 1.0 + 3 * u, -(1.0 + u)], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0 + 4 * u, -1.0], dtype=torch.float64)
    assert torch.equal(R.round_once(one, dtype), want) and torch.equal(R.round_to(one.float(), dtype).double(), want)
    # just above a tie, by less than fp32 resolves: one rounding goes up, two roundings land on the tie and go to even
    y = torch.tensor([1.0 + u + 2.0 ** -30], dtype=torch.float64)
    assert float(R.round_once(y, dtype)) == 1.0 + 2 * u and float(R.round_to(y.float(), dtype)) == 1.0
    if dtype == "fp16":                                                      # gradual underflow: spacing 2^-24 below 2^-14
        sub = torch.tensor([2.0 ** -15 + 2.0 ** -25 + 2.0 ** -40, 2.0 ** -24 * 0.49], dtype=torch.float64)
        assert torch.equal(R.round_once(sub, dtype), torch.tensor([2.0 ** -15 + 2.0 ** -24, 0.0], dtype=torch.float64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_fold_weights_candidates(dtype):
    """The two candidates of (T)(w * sc) -- the exact product rounded once, or the fp32 product rounded again -- are both within u of
    the exact product, differ in about one weight of 2^13 (fp16) / 2^16 (bf16), by exactly one ulp, and dw is that difference."""
    g = torch.Generator().manual_seed(2)
    w = torch.randn(256, 64, 1, 8, 8, generator=g) / 24
    sc = 1 + 0.2 * torch.randn(256, generator=g)
    wf, dw = R.fold_weights(w, sc, dtype)
    exact = w.double() * sc.double().reshape(-1, 1, 1, 1, 1)
    half_ulp = (R.U[dtype] * exact.abs() * (1 + 2.0 ** -20)).clamp_min(2.0 ** -25 if dtype == "fp16" else 0.0)   # fp16: gradual underflow
    assert bool(((wf.double() - exact).abs() <= half_ulp).all())
    if dtype == "fp32":
        assert not bool(dw.any()) and torch.equal(wf, exact.float())
        return
    assert torch.equal(R.round_to(wf, dtype), wf)
    n = int((dw > 0).sum())
    expect = w.numel() * 2.0 ** (-13 if dtype == "fp16" else -16)
    print(f"{dtype}: {n} of {w.numel()} weights ambiguous (expected about {expect:.0f})")
    assert expect / 4 < n < expect * 4
    other = torch.where(dw > 0, torch.where(R.round_to(wf + dw, dtype) == R.round_once(exact, dtype).float(), wf + dw, wf - dw), wf)
    amb = dw > 0
    assert torch.equal(R.round_to(other, dtype), other)                                           # the other candidate is representable
    ulp = 2.0 ** (torch.floor(torch.log2(exact.abs())) - (10 if dtype == "fp16" else 7))
    assert bool((dw[amb].double() == ulp[amb]).all())                                             # one ulp apart
    once, twice = (wf, other) if dtype == "fp16" else (other, wf)
    assert bool(((once.double() - exact).abs() <= (twice.double() - exact).abs())[amb].all())     # one rounding is the nearer one


# ---------------------------------------------------------------------------------------------------------------------------------
# a correct kernel passes
# ---------------------------------------------------------------------------------------------------------------------------------
def make_case(layer: R.Layer, shape, dtype: str, with_res: bool, seed: int):
    """(x, w_folded, shift, dw, res) of one convolution on random operands, rounded the way the engine's are."""
    g = torch.Generator().manual_seed(seed)
    n, t, h, w = shape
    x = R.round_to(torch.randn(n, layer.cin, t, h, w, generator=g).clamp_min(-0.5), dtype)          # post-ReLU-like, some negatives
    wt = torch.randn(layer.cout, layer.cin, *layer.kernel, generator=g) / math.sqrt(layer.K)
    sc, shift = R.fold_bn(1 + 0.2 * torch.randn(layer.cout, generator=g), 0.1 * torch.randn(layer.cout, generator=g),
                          0.3 * torch.randn(layer.cout, generator=g), torch.rand(layer.cout, generator=g) + 0.5)
    wf, dw = R.fold_weights(wt, sc, dtype)
    ho, wo = R.out_hw(h, w, layer)
    res = R.round_to(torch.randn(n, layer.cout, t, ho, wo, generator=g), dtype) if with_res else None
    return x, wf, shift, dw, res


def L(kernel, stride, cin, cout, relu=True):
    return R.Layer("case", "bn", "src", None, relu, kernel, stride, cin, cout)


GEOMETRIES = [
    (L((1, 7, 7), 2, 3, 45), (2, 2, 13, 15)),            # the stem, odd extents
    (L((3, 1, 1), 1, 45, 64), (2, 4, 5, 6)),
    (L((3, 1, 1), 1, 144, 64), (1, 3, 5, 6)),
    (L((3, 1, 1), 1, 460, 256), (1, 3, 3, 4)),
    (L((1, 3, 3), 1, 64, 144), (1, 2, 9, 16)),
    (L((1, 3, 3), 1, 512, 1152), (1, 1, 4, 5)),
    (L((1, 3, 3), 2, 64, 230), (1, 2, 9, 11)),           # odd extents at stride 2
    (L((1, 3, 3), 2, 256, 921), (1, 1, 5, 7)),
    (L((1, 1, 1), 2, 64, 128, relu=False), (2, 2, 7, 9)),
    (L((1, 1, 1), 2, 256, 512, relu=False), (1, 2, 5, 5)),
]


@pytest.mark.parametrize("dtype", DTYPES)
def test_correct_emulation_passes_every_geometry(dtype):
    """Largest err/bound of a correct kernel, per dtype.  For the 16-bit types it is close to 1 BY CONSTRUCTION: round-to-nearest
    reaches u / (1 + u) of the value and u |ref| is the bound's leading term, so the bound is tight, not loose (0.99 bf16, 0.98 fp16
    here).  What the derivation must leave well below 1 is the accumulation part -- the error of the UNROUNDED fp32 result against
    c (K + 3) 2^-24 A alone -- which stays under 0.05 (16-bit operands: exact products) and 0.1 (fp32)."""
    worst, worst_acc = 0.0, 0.0
    for i, (layer, shape) in enumerate(GEOMETRIES):
        for with_res in (False, True):
            x, wf, shift, dw, res = make_case(layer, shape, dtype, with_res, 100 + i)
            ref, A = R.layer_ref(x, wf, shift, res, layer)
            out = R.emulate(x, wf, shift, res, layer, dtype)
            what = f"emulation {dtype} k={layer.kernel} s={layer.stride} cin={layer.cin} res={with_res}"
            r, _ = R.gate(out, ref, A, layer.K, dtype, what)            # no flip term: the emulation multiplies the nominal weights
            worst = max(worst, r)
            acc = (R.emulate(x, wf, shift, res, layer, "fp32").double() - ref).abs() / (R.gamma(layer.K, dtype) * A)
            worst_acc = max(worst_acc, float(acc.max()))
    print(f"{dtype}: largest err/bound of the correct emulation {worst:.3f}; accumulation part alone {worst_acc:.3f}")
    assert worst < 1.0 and worst_acc < 0.25


def test_emulated_network_passes_and_names_37_taps():
    from helpers import seeded_state
    from syncfusion_amd.onset_net import VideoOnsetNet

    layers = R.onset_layers()
    assert len(layers) == 37 and sum(l_.name.endswith("downsample.0") for l_ in layers) == 3
    state = seeded_state(VideoOnsetNet(pretrained=False), 5)
    x = torch.randn(2, 3, 2, 29, 35, generator=torch.Generator().manual_seed(5))
    for dtype in ("fp16", "bf16"):
        taps = R.emulate_taps(state, x, dtype)
        res = R.check_all_layers(state, x[[1]], {k: v[v.shape[0] // 2:] for k, v in taps.items()}, dtype, f"emulated net {dtype}", clips=[0])
        assert len(res) == 37
        taps["layer3.0.conv1.0.3"][7, 5] = float("nan")                 # an unwritten element of the NaN-filled tap buffer
        with pytest.raises(AssertionError, match="non-finite"):
            R.check_all_layers(state, x, taps, dtype, "poisoned")


@pytest.mark.parametrize("shape", [(2, 3, 45, 71), (2, 4, 112, 112)])
def test_checkpoint_like_state_stays_inside_the_fp16_range(shape):
    """The seed test_gpu_onset_layers.py uses: every activation of the emulated fp16 network below 65504 / 4, four exactly-zero
    folded channels per BatchNorm, variances over five decades."""
    from syncfusion_amd.onset_net import VideoOnsetNet
    from test_gpu_onset_layers import CKPT_SEED, FP16_RANGE

    n, t, h, w = shape
    state = R.checkpoint_like_state(VideoOnsetNet(pretrained=False), CKPT_SEED)
    for layer in R.onset_layers():
        wf, shift, _ = R.folded_operands(state, layer, "fp16")
        v = state[R.PREFIX + layer.bn + ".running_var"]
        assert int((wf.flatten(1).abs().amax(1) == 0).sum()) == 4 and 1e-3 <= float(v.min()) and float(v.max()) <= 1e2
        assert float(v.max() / v.min()) > 1e3 and float(state[R.PREFIX + layer.bn + ".running_mean"].abs().max()) <= 3.0
    x = torch.randn(n, 3, t, h, w, generator=torch.Generator().manual_seed(17 * h + w + 1))
    taps = R.emulate_taps(state, x, "fp16")
    top = max(float(v.abs().max()) for v in taps.values())
    print(f"checkpoint-like {shape}: largest |activation| {top:.1f}")
    assert all(bool(torch.isfinite(v).all()) for v in taps.values()) and 10.0 < top < FP16_RANGE


# ---------------------------------------------------------------------------------------------------------------------------------
# planted faults: each fails the per-element gate and passes the whole-tensor gate at the real tap size
# ---------------------------------------------------------------------------------------------------------------------------------
def conv(x, wf, shift, res, layer, dtype):
    return R.emulate(x, wf, shift, res, layer, dtype)


def fault_halo_column(x, wf, shift, res, layer, dtype, clean):
    """(1,3,3): the last column of the 8 x 14 patch at (0, 0) of frame 1 reads its right halo column (w = 14) from frame 0."""
    x2 = x.clone()
    x2[:, :, 1, :, 14] = x[:, :, 0, :, 14]
    out = clean.clone()
    out[0, :, 1, 0:8, 13] = conv(x2, wf, shift, res, layer, dtype)[0, :, 1, 0:8, 13]
    return out


def fault_last_frame_tap(x, wf, shift, res, layer, dtype, clean):
    """(3,1,1): in the final ragged 128-position block the t + 1 tap that reads the LAST frame is dropped (at t = T - 1 itself that tap
    is padding, so the fault shows in frame T - 2)."""
    n, c, t, h, w = clean.shape
    x2 = x.clone()
    x2[:, :, t - 1] = 0
    p0 = (h * w) // 128 * 128
    assert 0 < h * w - p0 < 128
    out = clean.clone().reshape(n, c, t, h * w)
    out[0, :, t - 2, p0:] = conv(x2, wf, shift, res, layer, dtype).reshape(n, c, t, h * w)[0, :, t - 2, p0:]
    return out.reshape(clean.shape)


def fault_residual_tile(x, wf, shift, res, layer, dtype, clean):
    """(3,1,1) + residual: one 32-position x 32-column output tile of one frame of one clip stored without the residual."""
    n, c, t, h, w = clean.shape
    out = clean.clone().reshape(n, c, t, h * w)
    out[0, 32:64, 1, 32:64] = conv(x, wf, shift, None, layer, dtype).reshape(n, c, t, h * w)[0, 32:64, 1, 32:64]
    return out.reshape(clean.shape)


def fault_split_columns(x, wf, shift, res, layer, dtype, clean):
    """(1,3,3), 288 outputs: the second launch of the column split (channels >= 192) writes one 16-row block one row off."""
    n, c, t, h, w = clean.shape
    rows = clean.permute(0, 2, 3, 4, 1).reshape(-1, c).clone()
    rows[16:32, 192:] = rows[17:33, 192:].clone()
    return rows.reshape(n, t, h, w, c).permute(0, 4, 1, 2, 3)


def fault_stem_bottom_row(x, wf, shift, res, layer, dtype, clean):
    """(1,7,7) stride 2 on an odd height: the bottom output row of one frame reads the last input row as zero."""
    assert x.shape[3] % 2 == 1
    x2 = x.clone()
    x2[:, :, :, -1] = 0
    out = clean.clone()
    out[0, :, 0, -1] = conv(x2, wf, shift, res, layer, dtype)[0, :, 0, -1]
    return out


FAULTS = {
    # name: (fault, layer, small shape, residual, rows of the real tap at 32 clips)
    "halo_column_from_previous_frame": (fault_halo_column, L((1, 3, 3), 1, 64, 144), (1, 2, 10, 18), False, N32_ROWS["layer1"]),
    "last_frame_tap_dropped_in_ragged_block": (fault_last_frame_tap, L((3, 1, 1), 1, 144, 64), (1, 3, 12, 16), False, N32_ROWS["layer1"]),
    "residual_skipped_for_one_tile": (fault_residual_tile, L((3, 1, 1), 1, 144, 64), (1, 2, 8, 12), True, N32_ROWS["layer1"]),
    "split_columns_from_neighbouring_row": (fault_split_columns, L((1, 3, 3), 1, 128, 288), (1, 1, 8, 8), False, N32_ROWS["layer2"]),
    "stem_bottom_halo_row_zero_on_odd_height": (fault_stem_bottom_row, L((1, 7, 7), 2, 3, 45), (1, 1, 29, 113), False, N32_ROWS["stem_odd"]),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(FAULTS))
def test_planted_fault_fails_the_gate_and_passes_the_whole_tensor_one(name, dtype):
    fault, layer, shape, with_res, real_rows = FAULTS[name]
    x, wf, shift, dw, res = make_case(layer, shape, dtype, with_res, 7)
    ref, A = R.layer_ref(x, wf, shift, res, layer)
    clean = R.emulate(x, wf, shift, res, layer, dtype)
    R.gate(clean, ref, A, layer.K, dtype, f"{name} {dtype} clean", flip=R.flip_term(x, dw, layer))
    bad = fault(x, wf, shift, res, layer, dtype, clean)
    touched = int((bad != clean).sum())
    assert touched > 0
    with pytest.raises(AssertionError, match="err/bound"):
        R.gate(bad, ref, A, layer.K, dtype, f"{name} {dtype} planted", flip=R.flip_term(x, dw, layer))   # the flip term does not hide it
    if dtype == "fp32":
        return      # the stage-level fp32 gate is 1e-4 and the kernels in question never run in fp32: nothing to show
    # The stage-level gate at the REAL tap: the fault touches the same elements whatever the batch, the rest of the 32-clip tap carries
    # the clean rounding error:  rel^2 = (n_real mean(e_clean^2) + sum over the touched (e_bad^2 - e_clean^2)) / (n_real mean(ref^2))
    n_real = real_rows * layer.cout
    e_clean, e_bad = (clean.double() - ref) ** 2, (bad.double() - ref) ** 2
    rel = math.sqrt((n_real * float(e_clean.mean()) + float((e_bad - e_clean).sum())) / (n_real * float((ref ** 2).mean())))
    rel_small = float(e_bad.sum().sqrt() / ref.norm())
    print(f"{name} {dtype}: {touched} elements touched; whole-tensor rel-L2 {rel:.3e} at the real tap ({n_real:.2e} elements; "
          f"{rel_small:.3e} on this small one), stage gate {ONSET_TAP_TOL[dtype]:.1e}")
    assert rel < ONSET_TAP_TOL[dtype]
