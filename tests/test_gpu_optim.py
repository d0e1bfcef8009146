"""GPU suite of the HIP optimizer stage (syncfusion_amd/optim.py -> sf_optim_adamw_step, csrc/optim.hip): the update and the global-norm
clipping against the fp64 statement in tests/optim_ref.py with torch's fused AdamW as the yardstick, state-dict interchange with torch, the
hyper-parameter array and table-rebuild rules, the step captured in ``GraphedTrainStep`` and ``fit_batches`` with ``Model(optimizer="hip")``.

One parameter set reaches every path of the kernels: element counts 1, 3, 4, 1023, CHUNK, CHUNK + 1, 3 CHUNK + 7, a (64, 48, 3) weight, a
parameter that is a view at an offset of one element (its gradient and moments are aligned: the chunk runs element by element), one whose
gradient AND moments sit at that offset too (16-byte body behind a scalar head), one whose gradient alone is offset (the norm pass's head),
a parameter without a gradient and a frozen one; two groups with their own lr / weight_decay; gradients at scales 1e-6, 1, 1e3."""
import copy

import numpy as np
import pytest
import torch

from optim_ref import AdamWRef, grad_norm

pytestmark = [pytest.mark.gpu, pytest.mark.autograd]

BETAS, EPS = (0.95, 0.999), 1e-6                        # the reference's (exp/train_diffusion_gh.yaml)
GROUPS = [dict(lr=1e-3, betas=BETAS, eps=EPS, weight_decay=1e-3), dict(lr=3e-3, betas=BETAS, eps=EPS, weight_decay=5e-2)]
SCALES = (1e-6, 1.0, 1e3)
ULP = 2.0 ** -23


def _shapes():
    from syncfusion_amd.optim import CHUNK

    return [(1,), (3,), (4,), (1023,), (CHUNK,), (CHUNK + 1,), (3 * CHUNK + 7,), (64, 48, 3), (1029,), (2053,), (517,), (11,), (6,)]


VIEW_P, VIEW_ALL, VIEW_G, NO_GRAD, FROZEN = 8, 9, 10, 11, 12      # indices into _shapes()


class ParamSet:
    """One copy of the parameter set on the GPU with its optimizer (``kind``: "hip" | "torch")."""

    def __init__(self, kind: str, device, masters, max_grad_norm=None):
        from syncfusion_amd.optim import AdamW

        self.kind, self.device, self.max_grad_norm = kind, device, max_grad_norm
        self.keep = []
        self.params = []
        for i, m in enumerate(masters):
            if i in (VIEW_P, VIEW_ALL):     # a view into a flat buffer, one element in: not 16-byte aligned
                p = torch.nn.Parameter(self._offset_view(m.to(device)))
            else:
                p = torch.nn.Parameter(m.to(device).clone())
            if i == FROZEN:
                p.requires_grad_(False)
            self.params.append(p)
        self.group_of = [i % 2 for i in range(len(masters))]
        groups = [dict(params=[p for p, gi in zip(self.params, self.group_of) if gi == k], lr=GROUPS[k]["lr"], weight_decay=GROUPS[k]["weight_decay"])
                  for k in range(2)]
        if kind == "hip":
            self.opt = AdamW(groups, betas=BETAS, eps=EPS, max_grad_norm=max_grad_norm)
            # moments at the parameter's own offset for one tensor (as a loaded state may be): the update's vector body behind a scalar head
            p = self.params[VIEW_ALL]
            self.opt.state[p] = dict(step=torch.zeros((), dtype=torch.float32, device=device), exp_avg=self._offset_view(torch.zeros_like(p)),
                                     exp_avg_sq=self._offset_view(torch.zeros_like(p)))
        else:
            self.opt = torch.optim.AdamW(groups, betas=BETAS, eps=EPS, fused=True)

    def _offset_view(self, t):
        flat = torch.zeros(t.numel() + 5, dtype=torch.float32, device=self.device)
        self.keep.append(flat)
        v = flat[1:1 + t.numel()].view(t.shape)
        v.copy_(t.detach())
        assert v.data_ptr() % 16 == 4
        return v

    def set_grads(self, grads, fresh=True):
        old = [p.grad for p in self.params]
        for i, (p, g) in enumerate(zip(self.params, grads)):
            if g is None:
                p.grad = None
            elif not fresh and p.grad is not None:
                p.grad.copy_(g)
            elif i in (VIEW_ALL, VIEW_G) and self.kind == "hip":
                p.grad = self._offset_view(g.to(self.device))
            else:
                p.grad = g.to(self.device).clone()
        return old

    def step(self):
        if self.kind == "torch" and self.max_grad_norm is not None:
            torch.nn.utils.clip_grad_norm_([p for p in self.params if p.grad is not None], self.max_grad_norm)
        self.opt.step()


def _masters(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in _shapes()]


def _grads(gen):
    """Gradients of one step: scales 1e-6, 1, 1e3 across the tensors (v spans its range: sqrt(v) far below and far above eps)."""
    out = []
    for i, s in enumerate(_shapes()):
        out.append(None if i in (NO_GRAD, FROZEN) else torch.randn(s, generator=gen) * SCALES[i % 3])
    return out


def _ref(masters):
    return AdamWRef([m.numpy() for m in masters], GROUPS, [i % 2 for i in range(len(masters))])


def _np(grads):
    return [None if g is None else g.numpy() for g in grads]


def _err(x, x64) -> float:
    den = float(np.max(np.abs(x64)))
    num = float(np.max(np.abs(x.astype(np.float64) - x64)))
    return num / den if den > 0 else (0.0 if num == 0 else float("inf"))


def _gate(hip: ParamSet, tor: ParamSet, ref: AdamWRef, what=""):
    """e = max over tensors of max|X - X64| / max|X64| for p, exp_avg, exp_avg_sq;  e_hip <= 2 e_torch + 2^-23.  Both evaluate the same
    recurrence on fp32 storage: the factor 2 covers another contraction into fused multiply-adds, the additive term is one ulp for
    tensors where torch happens to be exact.  Step counters: equal exactly."""
    for name in ("p", "exp_avg", "exp_avg_sq"):
        e = {}
        for ps in (hip, tor):
            worst = 0.0
            for i, p in enumerate(ps.params):
                if ref.m[i] is None:
                    continue
                x = p if name == "p" else ps.opt.state[p][name]
                x64 = ref.p[i] if name == "p" else (ref.m[i] if name == "exp_avg" else ref.v[i])
                worst = max(worst, _err(x.detach().cpu().numpy(), x64))
            e[ps.kind] = worst
        print(f"{what} {name}: e_hip {e['hip']:.3e}  e_torch {e['torch']:.3e}  bound {2 * e['torch'] + ULP:.3e}")
        assert e["hip"] <= 2 * e["torch"] + ULP, (what, name, e)
    for i, p in enumerate(hip.params):
        if ref.m[i] is None:
            continue
        assert float(hip.opt.state[p]["step"]) == float(tor.opt.state[tor.params[i]]["step"]) == float(ref.steps[i]), i
        st = hip.opt.state[p]["step"]
        assert st.is_cuda and st.dtype == torch.float32 and st.dim() == 0


def _untouched(ps: ParamSet, masters):
    for i in (NO_GRAD, FROZEN):
        assert torch.equal(ps.params[i].detach().cpu(), masters[i]) and len(ps.opt.state.get(ps.params[i], {})) == 0, i


def test_update_against_fp64_with_torch_as_the_yardstick(cuda):
    masters = _masters(0)
    hip, tor, ref = ParamSet("hip", cuda, masters), ParamSet("torch", cuda, masters), _ref(masters)
    gen = torch.Generator().manual_seed(100)
    for it in range(4):
        grads = _grads(gen)
        hip.set_grads(grads)
        tor.set_grads(grads)
        hip.step()
        tor.step()
        ref.step(_np(grads))
        _gate(hip, tor, ref, f"step {it + 1}")
    assert hip.opt.last_grad_norm is None and float(hip.opt.last_clip_coef) == 1.0
    _untouched(hip, masters)
    assert ref.steps[0] == 4 and hip.opt.table_builds >= 1


@pytest.mark.parametrize("active", [True, False])
def test_clipping(cuda, active):
    masters = _masters(1)
    grads = _grads(torch.Generator().manual_seed(200))
    norm64 = grad_norm(_np(grads))
    max_norm = norm64 * (0.37 if active else 2.5)
    hip, tor, ref = ParamSet("hip", cuda, masters, max_norm), ParamSet("torch", cuda, masters, max_norm), _ref(masters)
    hip2 = ParamSet("hip", cuda, masters, max_norm)
    for ps in (hip, tor, hip2):
        ps.set_grads(grads)
    before = [None if p.grad is None else p.grad.clone() for p in hip.params]
    hip.step()
    tor.step()
    hip2.step()
    _, coef = ref.step(_np(grads), max_norm=max_norm)
    assert (coef < 1.0) == active
    # sum of squares as optim.hip accumulates it, fp32: per lane 16 (four accumulators over <= 16 float4) + 2 (their pairwise sum) + 2 (head
    # and tail elements) roundings in a row, then a tree over 256 lanes: log2(256) = 8; the fp64 sum over the chunks and the rounding of the
    # norm to fp32: + 2  ->  (20 + 8 + 2) * 2^-24 = 1.79e-6 relative on the sum, half of it, 8.94e-7, on the norm
    bound = (20 + 8 + 2) * 2.0 ** -24 / 2
    got = float(hip.opt.last_grad_norm)
    print(f"norm: hip {got!r}  fp64 {norm64!r}  rel {abs(got - norm64) / norm64:.3e}  bound {bound:.3e}")
    assert abs(got - norm64) <= bound * norm64
    assert abs(float(hip.opt.last_clip_coef) - coef) <= (bound + 2.0 ** -24) * coef
    for p, b in zip(hip.params, before):                 # .grad is not scaled (clip_grad_norm_ scales it in place)
        assert (p.grad is None and b is None) or torch.equal(p.grad, b)
    _gate(hip, tor, ref, f"clip active={active}")
    _untouched(hip, masters)
    for p, q in zip(hip.params, hip2.params):            # no atomics: the same step twice gives the same bits
        assert torch.equal(p, q)
    for p, q in zip(hip.params, hip2.params):
        if p in hip.opt.state:
            assert all(torch.equal(hip.opt.state[p][k], hip2.opt.state[q][k]) for k in ("step", "exp_avg", "exp_avg_sq"))
    assert float(hip.opt.last_grad_norm) == float(hip2.opt.last_grad_norm)


@pytest.mark.parametrize("direction", ["torch_to_hip", "hip_to_torch"])
def test_state_dict_round_trip(cuda, direction):
    masters = _masters(2)
    first_kind, second_kind = ("torch", "hip") if direction == "torch_to_hip" else ("hip", "torch")
    first, ref = ParamSet(first_kind, cuda, masters), _ref(masters)
    gen = torch.Generator().manual_seed(300)
    for _ in range(2):
        grads = _grads(gen)
        first.set_grads(grads)
        first.step()
        ref.step(_np(grads))
    second = ParamSet(second_kind, cuda, [p.detach().cpu() for p in first.params])
    if second_kind == "hip":
        second.opt.state.clear()
    second.opt.load_state_dict(copy.deepcopy(first.opt.state_dict()))
    assert isinstance(second.opt.state[second.params[0]]["step"], torch.Tensor)
    hip, tor = (second, first) if second_kind == "hip" else (first, second)
    for it in range(2):
        grads = _grads(gen)
        for ps in (first, second):
            ps.set_grads(grads)
            ps.step()
        ref.step(_np(grads))
        _gate(hip, tor, ref, f"{direction} step {it + 3}")
    assert ref.steps[0] == 4


def test_state_of_the_unfused_torch_optimizer_loads(cuda):
    """torch.optim.AdamW without fused keeps `step` as a host tensor: after load_state_dict the HIP class moves it to an fp32 device scalar."""
    from syncfusion_amd.optim import AdamW

    g = torch.Generator().manual_seed(5)
    w = torch.randn(300, generator=g)
    a, b = torch.nn.Parameter(w.to(cuda)), torch.nn.Parameter(w.to(cuda))
    plain = torch.optim.AdamW([a], lr=1e-3, betas=BETAS, eps=EPS, weight_decay=1e-2, foreach=False)
    ours = AdamW([b], lr=1e-3, betas=BETAS, eps=EPS, weight_decay=1e-2)
    ref = AdamWRef([w.numpy()], [dict(lr=1e-3, betas=BETAS, eps=EPS, weight_decay=1e-2)], [0])
    for it in range(3):
        gr = torch.randn(300, generator=g)
        a.grad = gr.to(cuda)
        plain.step()
        ref.step([gr.numpy()])
        if it == 0:
            assert not plain.state[a]["step"].is_cuda
            b.data.copy_(a.data)
            ours.load_state_dict(copy.deepcopy(plain.state_dict()))
        else:
            b.grad = gr.to(cuda)
            ours.step()
    st = ours.state[b]["step"]
    assert st.is_cuda and st.dtype == torch.float32 and float(st) == 3.0
    e_hip, e_torch = _err(b.detach().cpu().numpy(), ref.p[0]), _err(a.detach().cpu().numpy(), ref.p[0])
    assert e_hip <= 2 * e_torch + ULP, (e_hip, e_torch)


def test_hyper_parameter_change_without_a_table_rebuild(cuda):
    masters = _masters(3)
    hip, tor, ref = ParamSet("hip", cuda, masters), ParamSet("torch", cuda, masters), _ref(masters)
    gen = torch.Generator().manual_seed(400)
    for it in range(3):
        grads = _grads(gen)
        hip.set_grads(grads, fresh=False)       # the gradient tensors of the first step are refilled: the addresses stay
        tor.set_grads(grads)
        if it == 1:                             # as an LR scheduler does
            for ps in (hip, tor):
                ps.opt.param_groups[0]["lr"] *= 0.5
            ref.groups[0]["lr"] *= 0.5
            uploads = hip.opt.hyper_uploads
        hip.step()
        tor.step()
        ref.step(_np(grads))
        _gate(hip, tor, ref, f"lr change, step {it + 1}")
    assert hip.opt.table_builds == 1 and hip.opt.hyper_uploads == uploads + 1
    # the halved rate is what moved the parameters: a reference that kept the old one is far outside the gate
    stale = _ref(masters)
    gen = torch.Generator().manual_seed(400)
    for _ in range(3):
        stale.step(_np(_grads(gen)))
    assert _err(hip.params[4].detach().cpu().numpy(), stale.p[4]) > 100 * ULP


def test_table_rebuild_on_new_gradient_tensors(cuda):
    masters = _masters(4)
    hip, tor, ref = ParamSet("hip", cuda, masters), ParamSet("torch", cuda, masters), _ref(masters)
    gen = torch.Generator().manual_seed(500)
    grads = _grads(gen)
    hip.set_grads(grads)
    tor.set_grads(grads)
    hip.step()
    tor.step()
    ref.step(_np(grads))
    assert hip.opt.table_builds == 1
    grads = _grads(gen)
    old = hip.set_grads(grads, fresh=True)      # zero_grad(set_to_none=True) + backward: every .grad is a new allocation
    for o in old:                               # the old tensors stay alive (their addresses cannot be handed out again) and turn to garbage
        if o is not None:
            o.fill_(float("nan"))
    assert all(p.grad.data_ptr() != o.data_ptr() for p, o in zip(hip.params, old) if o is not None)
    tor.set_grads(grads)
    hip.step()
    tor.step()
    ref.step(_np(grads))
    assert hip.opt.table_builds == 2
    _gate(hip, tor, ref, "new gradient tensors")


def _small_model(cuda, seed, **kw):
    import functools

    from helpers import SMALL_ENCODER, SMALL_UNET
    from syncfusion_amd import DiffusionModel, Encoder1d, Model, RandomEmbedder, UNetV0, VDiffusion, VSampler

    torch.manual_seed(3)
    dm = DiffusionModel(net_t=functools.partial(UNetV0, seed=seed), diffusion_t=VDiffusion, sampler_t=VSampler, use_embedding_cfg=True, **SMALL_UNET)
    return Model(1e-3, 0.95, 0.999, 1e-6, 1e-3, dm, Encoder1d(seed=seed + 1, **SMALL_ENCODER), RandomEmbedder(SMALL_UNET["embedding_features"]), None,
                 **kw).to(cuda)


def test_optimizer_step_inside_the_graphed_train_step(cuda):
    """GraphedTrainStep(model, batch, optimizer=hip) -- forward, backward, clipping and AdamW in one graph -- against the eager
    training step + backward + the same optimizer class on a twin model: the same kernels in the same order, so every parameter and step
    counter is equal bit for bit after each of 3 steps; constructing the graph leaves the parameters where they were."""
    from syncfusion_amd.optim import AdamW
    from syncfusion_amd.training import GraphedTrainStep, training_step_scope

    ma, mb = _small_model(cuda, 5, optimizer="hip"), _small_model(cuda, 5, optimizer="hip")
    oa, ob = ma.configure_optimizers(), mb.configure_optimizers()
    assert isinstance(oa, AdamW) and isinstance(oa, torch.optim.AdamW)
    oa.max_grad_norm = ob.max_grad_norm = 0.05
    B, L0 = 2, 16 * 24
    g = torch.Generator().manual_seed(9)
    batches = [(torch.randn(B, 1, L0, generator=g).to(cuda), (torch.rand(B, 1, L0, generator=g) < 0.02).float().to(cuda)) for _ in range(3)]
    before = {k: p.detach().clone() for k, p in ma.named_parameters()}
    with pytest.raises(TypeError, match="syncfusion_amd.optim.AdamW"):
        GraphedTrainStep(ma, (batches[0][0], batches[0][1], batches[0][0], None, None),
                         optimizer=torch.optim.SGD([p for p in ma.parameters() if p.requires_grad], lr=1e-2))
    gs = GraphedTrainStep(ma, (batches[0][0], batches[0][1], batches[0][0], None, None), optimizer=oa)
    for k, p in ma.named_parameters():
        assert torch.equal(p, before[k]), f"constructing the graph moved {k}"
    assert all(float(st["step"]) == 0.0 and float(st["exp_avg"].abs().max()) == 0.0 for st in oa.state.values()) and len(oa.state) > 100
    for it, (x, y) in enumerate(batches):
        gs.sig.copy_(torch.rand(B, generator=g).to(cuda))
        gs.noise.copy_(torch.randn(B, 1, L0, generator=g).to(cuda))
        loss_g = float(gs.step((x, y, x, None, None), resample=False).detach())
        for p in mb.parameters():
            p.grad = None
        with training_step_scope():
            emb = mb.clap_encode_audio(x)
            _, info = mb.onsets_encoder(y, with_info=True)
            loss_e = mb.model(x, channels=info["xs"][2:-1], embedding=emb, sigmas=gs.sig.clone(), noise=gs.noise.clone())
            loss_e.backward()
        ob.step()
        assert float(loss_e) == loss_g
        assert float(ob.last_clip_coef) < 1.0, "the clip must be active for this check to mean something"
        assert float(oa.last_grad_norm) == float(ob.last_grad_norm)
        for (k, p), (_, q) in zip(ma.named_parameters(), mb.named_parameters()):
            assert torch.equal(p, q), (it, k)
            if q in ob.state:
                assert float(oa.state[p]["step"]) == float(ob.state[q]["step"]) == it + 1, (it, k)
    assert any(not torch.equal(p, before[k]) for k, p in ma.named_parameters())


def test_fit_batches_with_the_hip_optimizer(cuda):
    """The setting of the existing fit_batches test (2 micro-batches, gradient_clip_val 0.1, the clip active) with Model(optimizer="hip")
    against a second model stepped by hand with clip_grad_norm_ + torch's fused AdamW; the fp64 reference runs from the second model's
    accumulated gradients."""
    from syncfusion_amd.optim import AdamW
    from syncfusion_amd.training import fit_batches

    def batches():
        g = torch.Generator().manual_seed(61)
        out = []
        for _ in range(2):
            x = torch.randn(2, 1, 16 * 12, generator=g).to(cuda)
            y = (torch.rand(2, 1, 16 * 12, generator=g) < 0.05).float().to(cuda)
            out.append((x, y, x, None, None))
        return out

    a, b = _small_model(cuda, 3, optimizer="hip"), _small_model(cuda, 3)
    oa, ob = a.configure_optimizers(), b.configure_optimizers()
    assert isinstance(oa, AdamW) and type(ob) is torch.optim.AdamW
    torch.manual_seed(500)
    losses = fit_batches(a, oa, batches(), accumulate_grad_batches=2, gradient_clip_val=0.1)
    assert len(losses) == 2 and oa.max_grad_norm == 0.1
    torch.manual_seed(500)
    ob.zero_grad(set_to_none=True)
    for i, bt in enumerate(batches()):
        (b.training_step(bt, i) / 2).backward()
    owned = [p for group in ob.param_groups for p in group["params"]]
    ref = AdamWRef([p.detach().cpu().numpy() for p in owned], [dict(lr=1e-3, betas=(0.95, 0.999), eps=1e-6, weight_decay=1e-3)], [0] * len(owned))
    grads64 = [None if p.grad is None else p.grad.detach().cpu().numpy().astype(np.float64) for p in owned]
    norm = torch.nn.utils.clip_grad_norm_([p for p in b.parameters() if p.requires_grad], 0.1)
    assert float(norm) > 0.1, "the clip must be active for this check to mean something"
    ob.step()
    norm64, coef = ref.step(grads64, max_norm=0.1)
    assert coef < 1.0 and abs(float(oa.last_grad_norm) - norm64) <= 15 * 2.0 ** -24 * norm64
    owned_a = [p for group in oa.param_groups for p in group["params"]]
    e_hip = max(_err(p.detach().cpu().numpy(), r) for p, r, m in zip(owned_a, ref.p, ref.m) if m is not None)
    e_torch = max(_err(p.detach().cpu().numpy(), r) for p, r, m in zip(owned, ref.p, ref.m) if m is not None)
    print(f"fit_batches p: e_hip {e_hip:.3e}  e_torch {e_torch:.3e}  bound {2 * e_torch + ULP:.3e}")
    assert e_hip <= 2 * e_torch + ULP
    assert sum(m is not None for m in ref.m) > 100
