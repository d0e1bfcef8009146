"""Layer-isolated fp64 reference and per-element gate for the 37 convolutions of the VideoOnsetNet inference engine.

The stage-level tests (test_gpu_models.py) compare five whole tensors by rel-L2 after up to nine convolutions each; a kernel that is
wrong in a few thousand of 10^8 elements passes them.  Here every convolution k is checked on its own: the reference starts from the
DEVICE's tap of that convolution's input (and of its residual source), which are exact values of the engine's type carried in fp32, so
errors of earlier layers do not compound and a failure names one launch sequence.

Operands.  The engine folds the eval-mode BatchNorm into the weights at build time (csrc/misc.hip bn_fold_kernel, pack_conv_kernel,
called from onset_engine.cpp make_conv -> Packer::conv with nscale = the fold's scale):
    sc = g / sqrtf(v + eps);  shift = b - m * sc;  w_folded = (T)(w * sc)          all fp32, then ONE conversion to the engine type T
fold_bn / fold_weights restate it in the same fp32 order.  The library is built without fast-math flags and hipcc's default for HIP
device code is a correctly rounded fp32 divide and sqrt (the generated code is the div_scale / div_fmas / div_fixup sequence), so `sc`
is bit-equal to the IEEE value computed here (fold_bn forms it in fp64 and rounds, so that it does not depend on the host either).  Bit-equality of the folded 16-BIT WEIGHTS, however, CANNOT be guaranteed from the
source: under the compiler's default contraction (T)(w * sc) is either an fp32 multiply followed by a conversion (two roundings: what
the bf16 packer compiles to today) or one mixed-precision instruction that rounds the exact product once (v_fma_mixlo_f16: what the
fp16 packer compiles to today).  The two differ in about one weight of 2^13 (fp16) or 2^16 (bf16), by one ulp of the 16-bit type.  The
first GPU run of this gate found exactly that: one channel per fp16 convolution up to 4.9x over the bound, every other element
bit-equal to the rounded reference.  So fold_weights returns the weights of today's code generation as the nominal operand AND the
difference dw = |w_once - w_twice| to the other candidate, and the gate adds the flip term
    F_i = conv3d_fp64(|x|, dw)_i
for the (few) output channels that own such a weight.  It is the issue's one-ulp flip term 2 u_T max_k |w_k x_k| made exact -- zero
for every channel whose weights are unambiguous, ulp(w_k) |x_k| <= 2 u_T |w_k x_k| per ambiguous weight -- not a widened constant.
`shift` is NOT bit-pinned either: the compiler contracts b - m * sc into one fma.  It stays fp32 on both sides and differs by at most
one fp32 rounding of |shift|, which is the one unit of 2^-24 |shift| that (K + 3) leaves spare in the bound below (K products, bias,
residual: K + 2 roundings).
The stem's input is the caller's fp32 frames rounded to T (video_to_cl_kernel stores (T)x).

Gate, per element and with no element exempt:
    |dev_i - ref_i| <= u_T |ref_i| + c (K + 3) 2^-24 A_i  (+ F_i, see above)
    ref = act(conv3d_fp64(x, w_folded) + shift + res),   A = conv3d_fp64(|x|, |w_folded|) + |shift| + |res|
  * u_T |ref|: the one rounding of the stored output (unit roundoff 2^-8 bf16, 2^-11 fp16, 2^-24 fp32);
  * c (K + 3) 2^-24 A: the worst case of an fp32 accumulation of K = kt kh kw cin products plus bias, residual and activation in ANY
    order -- tile shape, column split and MFMA operand order need no allowance.  Products of 16-bit operands are exact in fp32; in the
    fp32 engine each product is rounded once with its add (fma).  ReLU is 1-Lipschitz.
  * c: the microarchitecture guide's matrix-core table says of the f32-input MFMA "exact f32 (== fmaf chain, bitwise)" and the HIP
    guide "bit-for-bit a k-ordered f32 fmaf chain ... one rounding per product, no wider internal accumulation": every add of the
    fp32 engine is round-to-nearest, c = 1.  Neither guide says how the 16-bit-input MFMA rounds the sum of its 16 products into the
    fp32 accumulator, so truncation is taken as possible there: c = 2.  That choice is not measured.
  * No launch sequence of the onset engine stores through an intermediate 16-bit rounding (the two launches of the column split write
    disjoint columns; the residual is read as stored and added in fp32), so SECOND_ROUNDING is empty.
  * fp16 outputs below 2^-14 are subnormal and their rounding error is up to 2^-25 rather than u |ref|.  No term is added for it: the
    accumulation term covers it wherever A >= 2^-25 / (c (K + 3) 2^-24), i.e. A >= 0.0037 at the smallest K of the network (64, the
    layer-2 shortcut) and A >= 0.0017 for the stem; a failure that this explains would show |ref| < 6.2e-5 in its message.

Plain module (not a conftest): the tests import it like helpers.py and numerics.py.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

U = {"fp32": 2.0 ** -24, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}          # unit roundoff of the stored type
C_ACC = {"fp32": 1, "bf16": 2, "fp16": 2}                                 # see the module docstring
U24 = 2.0 ** -24
TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SECOND_ROUNDING: Tuple[str, ...] = ()      # engine paths that store through an intermediate 16-bit rounding: none
BN_EPS = 1e-5
PREFIX = "net.model."
STAGES = (("layer1", 64, 1), ("layer2", 128, 2), ("layer3", 256, 2), ("layer4", 512, 2))


def round_to(x: torch.Tensor, dtype: str) -> torch.Tensor:
    """x rounded to the engine type (round-to-nearest-even), carried in fp32."""
    return x.float().to(TORCH_DT[dtype]).float()


def fold_bn(g, b, m, v, eps: float = BN_EPS):
    """(scale, shift) of bn_fold_kernel as IEEE fp32 values.  Every fp32 operation is formed in fp64 and rounded to fp32: for +, *,
    sqrt and / of fp32 operands that IS the correctly rounded fp32 result (53 >= 2 * 24 + 2 bits), whatever the host's vectorised
    fp32 kernels do -- torch's own fp32 `g / torch.sqrt(v + eps)` was found to differ between two hosts in the last bit of sc, which
    flips a 16-bit weight in about one of 2^13.  shift is the device's contracted form fma(-m, sc, b)."""
    g, b, m, v = (t.float().double() for t in (g, b, m, v))
    eps32 = torch.tensor(eps, dtype=torch.float32).double()
    s = (v + eps32).float().double()
    r = torch.sqrt(s).float().double()
    sc = (g / r).float()
    return sc, (b - m * sc.double()).float()


def round_once(y: torch.Tensor, dtype: str) -> torch.Tensor:
    """An fp64 tensor rounded ONCE to the engine type (round-to-nearest-even, gradual underflow), returned in fp64.  torch's own
    double -> half / bfloat16 conversions go through fp32, i.e. round twice."""
    if dtype == "fp32":
        return y.float().double()
    bits, emin = (11, -14) if dtype == "fp16" else (8, -126)
    _, e = torch.frexp(y)                                                # |y| = m 2^e, m in [0.5, 1)
    ulp = torch.ldexp(torch.ones_like(y), (e - 1).clamp_min(emin) - (bits - 1))
    return torch.round(y / ulp) * ulp                                    # exact scalings by powers of two; torch.round is half-to-even


def fold_weights(w: torch.Tensor, sc: torch.Tensor, dtype: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """pack_conv_kernel's (T)(w * scale[n]) -> (nominal folded weights, dw), both fp32 and of w's shape.  Nominal: what today's code
    generation stores (fp16: the exact product rounded once; bf16: fp32 product, then converted; fp32: the fp32 product).  dw >= 0: the
    distance to the other candidate, non-zero for the few weights where one and two roundings disagree."""
    sc = sc.float().reshape(-1, *([1] * (w.dim() - 1)))
    twice = round_to((w.double() * sc.double()).float(), dtype)              # the IEEE fp32 product, then the conversion
    if dtype == "fp32":
        return twice, torch.zeros_like(twice)
    once = round_once(w.double() * sc.double(), dtype).float()           # a product of two fp32 values is exact in fp64
    return (once if dtype == "fp16" else twice), (once - twice).abs()


class Layer:
    """One tapped convolution: geometry and where its operands come from."""

    def __init__(self, name, bn, src, res, relu, kernel, stride, cin, cout):
        self.name, self.bn, self.src, self.res, self.relu = name, bn, src, res, relu
        self.kernel, self.stride, self.cin, self.cout = kernel, stride, cin, cout
        self.padding = tuple(k // 2 for k in kernel)

    @property
    def K(self) -> int:
        return self.kernel[0] * self.kernel[1] * self.kernel[2] * self.cin

    def __repr__(self):
        return f"Layer({self.name}, k={self.kernel}, s={self.stride}, {self.cin}->{self.cout}, res={self.res})"


def midplanes(inp: int, planes: int) -> int:
    return (inp * planes * 27) // (inp * 9 + 3 * planes)


def onset_layers() -> List[Layer]:
    """The 37 convolutions in launch order; `src` / `res` name the tap they read ("input" = the frames)."""
    L = [Layer("stem.0", "stem.1", "input", None, True, (1, 7, 7), 2, 3, 45),
         Layer("stem.3", "stem.4", "stem.0", None, True, (3, 1, 1), 1, 45, 64)]
    x, cin = "stem.3", 64
    for stage, planes, stride in STAGES:
        for b in range(2):
            pre = f"{stage}.{b}"
            s = stride if b == 0 else 1
            inp = cin if b == 0 else planes
            mid = midplanes(inp, planes)
            L.append(Layer(pre + ".conv1.0.0", pre + ".conv1.0.1", x, None, True, (1, 3, 3), s, inp, mid))
            L.append(Layer(pre + ".conv1.0.3", pre + ".conv1.1", pre + ".conv1.0.0", None, True, (3, 1, 1), 1, mid, planes))
            L.append(Layer(pre + ".conv2.0.0", pre + ".conv2.0.1", pre + ".conv1.0.3", None, True, (1, 3, 3), 1, planes, mid))
            res = x
            if b == 0 and (s != 1 or inp != planes):
                L.append(Layer(pre + ".downsample.0", pre + ".downsample.1", x, None, False, (1, 1, 1), s, inp, planes))
                res = pre + ".downsample.0"
            L.append(Layer(pre + ".conv2.0.3", pre + ".conv2.1", pre + ".conv2.0.0", res, True, (3, 1, 1), 1, mid, planes))
            x = pre + ".conv2.0.3"
        cin = planes
    return L


def folded_operands(state: Dict[str, torch.Tensor], layer: Layer, dtype: str):
    """(w_folded fp32 in the engine type's values, shift fp32, dw) of one convolution from a VideoOnsetNet state_dict."""
    p = PREFIX + layer.bn
    sc, shift = fold_bn(state[p + ".weight"], state[p + ".bias"], state[p + ".running_mean"], state[p + ".running_var"])
    wf, dw = fold_weights(state[PREFIX + layer.name + ".weight"], sc, dtype)
    return wf, shift, dw


def flip_term(x: torch.Tensor, dw: torch.Tensor, layer: Layer) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
    """(channels, F): F = conv3d_fp64(|x|, dw) for the output channels that own a weight whose 16-bit rounding is ambiguous; None when
    there is none."""
    ch = (dw.flatten(1).amax(1) > 0).nonzero().flatten()
    if ch.numel() == 0:
        return None
    return ch, F.conv3d(x.double().abs(), dw[ch].double(), None, stride=(1, layer.stride, layer.stride), padding=layer.padding)


def rows_to_ncthw(rows: torch.Tensor, n: int, t: int, h: int, w: int) -> torch.Tensor:
    """An engine tap (n * t * h * w rows ordered ((n t) h) w, C) -> (n, C, t, h, w)."""
    return rows.reshape(n, t, h, w, rows.shape[1]).permute(0, 4, 1, 2, 3)


def out_hw(h: int, w: int, layer: Layer) -> Tuple[int, int]:
    (_, kh, kw), (_, ph, pw), s = layer.kernel, layer.padding, layer.stride
    return (h + 2 * ph - kh) // s + 1, (w + 2 * pw - kw) // s + 1


def layer_ref(x: torch.Tensor, w: torch.Tensor, shift: torch.Tensor, res: Optional[torch.Tensor], layer: Layer):
    """(ref, A) in fp64 from (n, C, t, h, w) operands: ref = act(conv + shift + res), A = conv(|x|, |w|) + |shift| + |res|."""
    kw = dict(stride=(1, layer.stride, layer.stride), padding=layer.padding)
    xd, wd, sd = x.double(), w.double(), shift.double().reshape(1, -1, 1, 1, 1)
    ref = F.conv3d(xd, wd, None, **kw)
    ref += sd
    A = F.conv3d(xd.abs_(), wd.abs(), None, **kw)     # xd is not used again
    A += sd.abs()
    if res is not None:
        rd = res.double()
        ref += rd
        A += rd.abs_()
    if layer.relu:
        ref.clamp_(min=0.0)
    return ref, A


def gamma(layer_K: int, dtype: str) -> float:
    return C_ACC[dtype] * (layer_K + 3) * U24


def bound_of(ref: torch.Tensor, A: torch.Tensor, K: int, dtype: str, roundings: int = 1, flip=None) -> torch.Tensor:
    b = (roundings * U[dtype]) * ref.abs() + gamma(K, dtype) * A
    if flip is not None:
        b[:, flip[0]] += flip[1]
    return b


def gate(dev: torch.Tensor, ref: torch.Tensor, A: torch.Tensor, K: int, dtype: str, what: str,
         clips: Optional[Sequence[int]] = None, path: Optional[str] = None, flip=None) -> Tuple[float, float]:
    """Assert |dev - ref| <= u |ref| + c (K + 3) 2^-24 A (+ F on the channels of `flip`, flip_term's result) for EVERY element of (n, C, t, h, w) tensors (dev finite everywhere: the tap
    buffer is NaN-filled, an unwritten row fails).  Prints and returns (max err / bound, whole-tensor rel-L2); the failure names the
    worst element as (clip, frame, h, w, channel).  `clips`: the batch indices of dev's clips; `path`: the launch sequence, which
    earns a second output rounding only if it is listed in SECOND_ROUNDING."""
    d = dev.detach().double().cpu()
    assert d.shape == ref.shape == A.shape, f"{what}: shapes {tuple(d.shape)} / {tuple(ref.shape)} / {tuple(A.shape)}"

    def where(flat_idx: int) -> str:
        n, c, t, h, w = _unravel(flat_idx, d.shape)
        clip = clips[n] if clips is not None else n
        return (f"(clip {clip}, frame {t}, h {h}, w {w}, channel {c}): got {float(d[n, c, t, h, w]):.9g}, "
                f"ref {float(ref[n, c, t, h, w]):.9g}, A {float(A[n, c, t, h, w]):.4g}")

    bad = ~torch.isfinite(d)
    if bool(bad.any()):
        raise AssertionError(f"{what}: {int(bad.sum())} non-finite outputs of {d.numel()}, first at {where(int(bad.flatten().nonzero()[0]))}")
    err = (d - ref).abs_()
    rel = float(err.norm() / ref.norm().clamp_min(1e-300))
    bound = bound_of(ref, A, K, dtype, 2 if path in SECOND_ROUNDING else 1, flip)
    # err / bound with 0 / 0 = 0 (an exactly-zero folded channel must come back exactly) and x / 0 = inf
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = int(ratio.flatten().argmax())
    r = float(ratio.flatten()[worst])
    print(f"{what}: err/bound {r:.3f}, rel-L2 {rel:.3e}, K {K}, {d.numel()} elements" + (f", {path}" if path else "")
          + (f", flip term on {flip[0].numel()} channels" if flip is not None else ""))
    assert r <= 1.0, (f"{what}: err/bound {r:.3f} > 1 at {where(worst)}; {int((ratio > 1).sum())} of {d.numel()} elements over the "
                      f"bound, rel-L2 {rel:.3e}" + (f", path {path}" if path else ""))
    return r, rel


def _unravel(i: int, shape) -> tuple:
    out = []
    for s in reversed(shape):
        out.append(i % s)
        i //= s
    return tuple(reversed(out))


def emulate(x: torch.Tensor, w: torch.Tensor, shift: torch.Tensor, res: Optional[torch.Tensor], layer: Layer, dtype: str) -> torch.Tensor:
    """What a correct kernel computes: the same rounded operands, conv3d accumulated in fp32, bias / residual / ReLU in fp32, the
    output rounded once to the engine type."""
    y = F.conv3d(x.float(), w.float(), None, stride=(1, layer.stride, layer.stride), padding=layer.padding)
    y = y + shift.float().reshape(1, -1, 1, 1, 1)
    if res is not None:
        y = y + res.float()
    if layer.relu:
        y = y.clamp_min(0.0)
    return round_to(y, dtype)


def emulate_taps(state, x: torch.Tensor, dtype: str) -> Dict[str, torch.Tensor]:
    """CPU stand-in for the engine's detail taps: the 37 emulated convolutions chained, as (rows, C) fp32 tensors."""
    acts, taps = {"input": round_to(x, dtype)}, {}
    for layer in onset_layers():
        wf, shift, _ = folded_operands(state, layer, dtype)
        y = emulate(acts[layer.src], wf, shift, acts[layer.res] if layer.res else None, layer, dtype)
        acts[layer.name] = y
        taps[layer.name] = y.permute(0, 2, 3, 4, 1).reshape(-1, layer.cout)
    return taps


def checkpoint_like_state(module: torch.nn.Module, seed: int) -> Dict[str, torch.Tensor]:
    """A state that looks like a trained checkpoint rather than an initialisation: running variances log-uniform in [1e-3, 1e2],
    running means up to +-3, and four channels per BatchNorm with weight = 0 (the folded weights of those channels are exactly zero and
    the layer's output there is act(shift + res)).  Convolution weights are scaled by sqrt(running_var) of their BatchNorm so that the
    pre-normalisation activations have about the variance the BatchNorm is said to have tracked; a mean of 3 over a standard deviation
    of 0.03 still shifts a channel by 100, so activations reach the hundreds and shift cancels against the convolution (A >> |ref|)."""
    import math

    from helpers import seeded_state

    st = seeded_state(module, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    for layer in onset_layers():
        p = PREFIX + layer.bn
        c = st[p + ".running_var"].numel()
        lv = torch.rand(c, generator=gen) * (math.log(1e2) - math.log(1e-3)) + math.log(1e-3)
        var = torch.exp(lv)
        st[p + ".running_var"] = var
        st[p + ".running_mean"] = torch.rand(c, generator=gen) * 6.0 - 3.0
        dead = torch.randperm(c, generator=gen)[:4]
        st[p + ".weight"][dead] = 0.0
        wn = PREFIX + layer.name + ".weight"
        st[wn] = st[wn] * var.sqrt().reshape(-1, 1, 1, 1, 1)
    return st


def check_all_layers(state, x: torch.Tensor, taps: Dict[str, torch.Tensor], dtype: str, what: str, clips: Optional[Sequence[int]] = None,
                     paths: Optional[Dict[str, str]] = None, max_abs: Optional[float] = None) -> Dict[str, Tuple[float, float]]:
    """Run every convolution tap of one forward through the gate.  x: the (N, 3, T, H, W) frames on the CPU; taps: the engine's
    detail taps (restricted to `clips` when given).  max_abs: assert first, from the fp64 reference, that no activation exceeds it.
    Returns {tap: (err/bound, rel-L2)}; every tap is checked before the first failure is raised."""
    sel = list(clips) if clips is not None else list(range(x.shape[0]))
    n, t = len(sel), x.shape[2]
    hw = {"input": (x.shape[3], x.shape[4])}
    acts = {"input": round_to(x[sel], dtype)}
    out, failures = {}, []
    for layer in onset_layers():
        assert layer.name in taps, f"{what}: no tap named {layer.name}"
        h, w = hw[layer.src]
        ho, wo = out_hw(h, w, layer)
        hw[layer.name] = (ho, wo)
        dev_rows = taps[layer.name].cpu()
        assert tuple(dev_rows.shape) == (n * t * ho * wo, layer.cout), f"{what} {layer.name}: tap shape {tuple(dev_rows.shape)}"
        acts[layer.name] = rows_to_ncthw(dev_rows, n, t, ho, wo)
        wf, shift, dw = folded_operands(state, layer, dtype)
        ref, A = layer_ref(acts[layer.src], wf, shift, acts[layer.res] if layer.res else None, layer)
        flip = flip_term(acts[layer.src], dw, layer)
        if max_abs is not None:
            assert float(ref.abs().max()) <= max_abs, f"{what} {layer.name}: |activation| reaches {float(ref.abs().max()):.4g} > {max_abs:.4g}"
        try:
            out[layer.name] = gate(acts[layer.name], ref, A, layer.K, dtype, f"{what} {layer.name}", sel, paths.get(layer.name) if paths else None, flip)
        except AssertionError as e:      # keep going: the pattern over the taps is the evidence
            failures.append(str(e))
        del ref, A
    assert len(out) + len(failures) == 37
    assert not failures, f"{len(failures)} of 37 taps over the bound:\n" + "\n".join(failures)
    return out
