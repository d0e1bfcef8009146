"""CPU suite of the HIP optimizer stage (syncfusion_amd/optim.py, sf_optim_adamw_step): the fp64 reference the GPU tests lean on against
torch itself, the descriptor table's layout against hand-computed values, when the table is rebuilt, the fallback on CPU parameters, the
``optimizer`` init-arg of both ``Model`` classes and the host-side argument checks of the C entry point.  No kernel runs here."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

from helpers import ROOT
from optim_ref import AdamWRef, clip_coef, grad_norm


def test_optim_ref_equals_torch_adamw_in_float64():
    """5 steps, two groups with their own lr / weight_decay, one parameter without a gradient on steps 2-3, clipping active on some steps and
    not on others: the numpy statement and torch.optim.AdamW (CPU, float64) differ by association order in fp64 only -> rtol 1e-12."""
    g = torch.Generator().manual_seed(11)
    shapes = [(7,), (5, 3), (1,), (4, 2, 3), (33,)]
    masters = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
    groups = [dict(lr=1e-3, betas=(0.95, 0.999), eps=1e-6, weight_decay=1e-3), dict(lr=3e-3, betas=(0.95, 0.999), eps=1e-6, weight_decay=5e-2)]
    group_of = [0, 1, 0, 1, 1]
    params = [torch.nn.Parameter(m.clone()) for m in masters]
    opt = torch.optim.AdamW([dict(params=[p for p, gi in zip(params, group_of) if gi == k], lr=groups[k]["lr"], weight_decay=groups[k]["weight_decay"])
                             for k in range(2)], betas=(0.95, 0.999), eps=1e-6)
    ref = AdamWRef([m.numpy() for m in masters], groups, group_of)
    max_norms = [1e9, 0.5, 1e9, 0.25, 2.0]        # steps 1 and 3: far above any norm (inactive); steps 2, 4, 5: below it (active)
    active = []
    for it in range(5):
        grads = [torch.randn(s, generator=g, dtype=torch.float64) * (10.0 if it % 2 else 1.0) for s in shapes]
        present = [not (i == 3 and it in (1, 2)) for i in range(len(shapes))]
        for p, gr, has in zip(params, grads, present):
            p.grad = gr.clone() if has else None
        norm_t = torch.nn.utils.clip_grad_norm_(params, max_norms[it])
        opt.step()
        norm_r, coef = ref.step([gr.numpy() for gr in grads], present, max_norm=max_norms[it])
        active.append(coef < 1.0)
        np.testing.assert_allclose(norm_r, float(norm_t), rtol=1e-12)
        assert norm_r == grad_norm([gr.numpy() for gr in grads], present) and coef == clip_coef(norm_r, max_norms[it])
        for i, p in enumerate(params):
            np.testing.assert_allclose(ref.p[i], p.detach().numpy(), rtol=1e-12, atol=0, err_msg=f"p[{i}] step {it + 1}")
            if ref.m[i] is not None:
                np.testing.assert_allclose(ref.m[i], opt.state[p]["exp_avg"].numpy(), rtol=1e-12, atol=0)
                np.testing.assert_allclose(ref.v[i], opt.state[p]["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
                assert ref.steps[i] == int(opt.state[p]["step"])
    assert active == [False, True, False, True, True]
    assert ref.steps == [5, 5, 5, 3, 5]


def test_chunk_size_is_the_headers():
    from syncfusion_amd import optim

    header = open(os.path.join(ROOT, "include", "syncfusion_amd.h")).read()
    assert int(re.search(r"#define\s+SF_OPTIM_CHUNK\s+(\d+)", header).group(1)) == optim.CHUNK
    assert optim.CHUNK % 4 == 0


def test_table_layout_against_hand_computed_values():
    from syncfusion_amd.optim import CHUNK, DESC_WORDS, build_table, chunks_of

    numels = [1, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5]
    assert [chunks_of(n) for n in numels] == [1, 1, 1, 1, 2, 3]
    groups = [0, 1, 1, 0, 2, 1]
    records = [(0x1000 * (i + 1), 0x2000 * (i + 1), 0x3000 * (i + 1), 0x4000 * (i + 1), 0x5000 * (i + 1), n, gi) for i, (n, gi) in enumerate(zip(numels, groups))]
    table, total = build_table(records)
    assert total == 9 and table.dtype == torch.int64 and tuple(table.shape) == (6, DESC_WORDS) and table.is_contiguous()
    assert [int(w) >> 32 for w in table[:, 6]] == [0, 1, 2, 3, 4, 6]                       # first_chunk: the running sum
    assert [int(w) & 0xFFFFFFFF for w in table[:, 6]] == groups
    assert table[:, 5].tolist() == numels and table[:, 7].tolist() == [0] * 6
    for i in range(6):
        assert table[i, :5].tolist() == [0x1000 * (i + 1), 0x2000 * (i + 1), 0x3000 * (i + 1), 0x4000 * (i + 1), 0x5000 * (i + 1)]
    with pytest.raises(ValueError):
        build_table([(1, 2, 3, 4, 5, 0, 0)])
    # an address in the upper half of the 64-bit range keeps its bits in the signed table
    t2, _ = build_table([((1 << 63) + 16, 2, 3, 4, 5, 1, 0)])
    assert int(t2[0, 0]) & 0xFFFFFFFFFFFFFFFF == (1 << 63) + 16


def _cpu_optimizer():
    from syncfusion_amd.optim import AdamW

    g = torch.Generator().manual_seed(3)
    a, b, c = (torch.nn.Parameter(torch.randn(n, generator=g)) for n in (5, 40000, 9))
    opt = AdamW([dict(params=[a, b], lr=1e-3, weight_decay=0.0), dict(params=[c], lr=2e-3, weight_decay=1e-2)], betas=(0.95, 0.999), eps=1e-6)
    return opt, (a, b, c)


def test_table_is_rebuilt_only_when_an_address_changes():
    """``_prepare`` (state, table, hyper-parameter array: everything in front of the launch) works on any device; the table follows the
    (p, g) addresses, the hyper-parameter array its values."""
    from syncfusion_amd.optim import CHUNK

    opt, (a, b, c) = _cpu_optimizer()
    a.grad, c.grad = torch.ones_like(a), torch.ones_like(c)            # b has no gradient: it is not listed
    opt._prepare(opt._entries())
    assert opt.table_builds == 1 and opt.hyper_uploads == 1
    assert opt._table_dev.shape == (2, 8) and opt._total_chunks == 2
    assert opt._table_dev[:, 0].tolist() == [a.data_ptr(), c.data_ptr()] and opt._table_dev[:, 1].tolist() == [a.grad.data_ptr(), c.grad.data_ptr()]
    assert [int(w) & 0xFFFFFFFF for w in opt._table_dev[:, 6]] == [0, 1]
    assert opt._table_dev[0, 2] == opt.state[a]["exp_avg"].data_ptr() and opt._table_dev[0, 4] == opt.state[a]["step"].data_ptr()
    assert opt.state[a]["step"].dtype == torch.float32 and opt.state[a]["step"].dim() == 0 and b not in opt.state
    a.grad.mul_(2.0)                                                  # new values, the same tensors
    opt._prepare(opt._entries())
    assert opt.table_builds == 1 and opt.hyper_uploads == 1
    opt.param_groups[0]["lr"] = 5e-4                                  # a scheduler: the array follows, the table stays
    opt._prepare(opt._entries())
    assert opt.table_builds == 1 and opt.hyper_uploads == 2 and opt._hyper_dev.dtype == torch.float64
    assert opt._hyper_dev[8:13].tolist() == [5e-4, 0.95, 0.999, 1e-6, 0.0] and opt._hyper_dev[16:21].tolist() == [2e-3, 0.95, 0.999, 1e-6, 1e-2]
    opt.max_grad_norm = 0.5
    opt._prepare(opt._entries())
    assert opt.hyper_uploads == 3 and float(opt._hyper_dev[0]) == 0.5 and opt.table_builds == 1
    keep = a.grad
    a.grad = torch.ones_like(a)                                       # a fresh allocation, as zero_grad(set_to_none=True) + backward
    assert a.grad.data_ptr() != keep.data_ptr()
    opt._prepare(opt._entries())
    assert opt.table_builds == 2 and int(opt._table_dev[0, 1]) == a.grad.data_ptr()
    b.grad = torch.ones_like(b)                                       # one more tensor: three records, b's three chunks in between
    opt._prepare(opt._entries())
    assert opt.table_builds == 3 and opt._total_chunks == 1 + (40000 + CHUNK - 1) // CHUNK + 1
    assert [int(w) >> 32 for w in opt._table_dev[:, 6]] == [0, 1, 4]


def test_cpu_parameters_fall_back_to_torch_with_one_warning():
    opt, (a, b, c) = _cpu_optimizer()
    assert isinstance(opt, torch.optim.AdamW)
    twin = [torch.nn.Parameter(p.detach().clone()) for p in (a, b, c)]
    ref = torch.optim.AdamW([dict(params=twin[:2], lr=1e-3, weight_decay=0.0), dict(params=twin[2:], lr=2e-3, weight_decay=1e-2)], betas=(0.95, 0.999),
                            eps=1e-6)
    g = torch.Generator().manual_seed(4)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for _ in range(3):
            for p, q in zip((a, b, c), twin):
                p.grad = torch.randn(p.shape, generator=g)
                q.grad = p.grad.clone()
            opt.step()
            ref.step()
    ours = [w for w in seen if "syncfusion_amd.optim.AdamW" in str(w.message)]
    assert len(ours) == 1 and "torch.optim.AdamW.step" in str(ours[0].message)
    assert opt.table_builds == 0 and opt.last_grad_norm is None
    for p, q in zip((a, b, c), twin):
        assert torch.equal(p, q)
    # the state is torch's own layout and loads into a plain torch.optim.AdamW
    sd = opt.state_dict()
    assert set(sd["state"][0].keys()) == {"step", "exp_avg", "exp_avg_sq"}
    ref.load_state_dict(sd)


def test_configure_optimizers_keeps_torch_unless_hip_on_a_gpu():
    import functools

    import syncfusion_amd as sa
    from helpers import SMALL_ENCODER, SMALL_UNET
    from syncfusion_amd.optim import AdamW

    def diffusion_model(**kw):
        dm = sa.DiffusionModel(net_t=functools.partial(sa.UNetV0, seed=1), diffusion_t=sa.VDiffusion, sampler_t=sa.VSampler, use_embedding_cfg=True,
                               **SMALL_UNET)
        return sa.Model(1e-3, 0.95, 0.999, 1e-6, 1e-3, dm, sa.Encoder1d(seed=2, **SMALL_ENCODER), sa.RandomEmbedder(SMALL_UNET["embedding_features"]), None, **kw)

    for make in (diffusion_model, lambda **kw: sa.OnsetModel(1e-4, 0.9, 0.999, 1e-8, 1e-2, sa.VideoOnsetNet(False), **kw)):
        for kw in ({}, dict(optimizer="torch"), dict(optimizer="hip")):   # CPU parameters: the plain torch class whatever was asked for
            opt = make(**kw).configure_optimizers()
            assert type(opt) is torch.optim.AdamW and not isinstance(opt, AdamW)
        with pytest.raises(ValueError, match="optimizer"):
            make(optimizer="lion")


def test_c_entry_point_refuses_bad_arguments_on_the_host():
    """Null table, n_tensors <= 0, a short workspace and clip outside {0, 1} are refused before anything is launched (no device is touched:
    the pointers are host addresses)."""
    from syncfusion_amd import _lib

    lib = _lib.load()
    assert lib.sf_optim_workspace_bytes(0) == -1 and lib.sf_optim_workspace_bytes(-3) == -1
    need = lib.sf_optim_workspace_bytes(5)
    assert need >= 5 * (4 + 16) and lib.sf_optim_workspace_bytes(6) > need
    buf = torch.zeros(4096, dtype=torch.float64)
    p = buf.data_ptr()
    assert p % 16 == 0
    assert lib.sf_optim_adamw_step(None, 2, 5, p, 1, 1, p, p, need, None) != 0
    assert b"null" in lib.sf_last_error()
    assert lib.sf_optim_adamw_step(p, 2, 5, None, 1, 1, p, p, need, None) != 0 and b"null" in lib.sf_last_error()
    assert lib.sf_optim_adamw_step(p, 0, 5, p, 1, 1, p, p, need, None) != 0
    assert b"n_tensors" in lib.sf_last_error()
    assert lib.sf_optim_adamw_step(p, 2, 5, p, 1, 1, p, p, need - 1, None) != 0
    assert b"workspace" in lib.sf_last_error()
    assert lib.sf_optim_adamw_step(p, 2, 5, p, 1, 2, p, p, need, None) != 0
    assert b"clip" in lib.sf_last_error()
    assert lib.sf_optim_adamw_step(p, 2, 5, p, 1, -1, p, p, need, None) != 0 and b"clip" in lib.sf_last_error()
    assert lib.sf_optim_adamw_step(p, 6, 5, p, 1, 0, p, p, need, None) != 0            # fewer chunks than tensors
    assert b"total_chunks" in lib.sf_last_error()
    assert lib.sf_optim_adamw_step(p, 2, 5, p, 0, 0, p, p, need, None) != 0 and b"n_groups" in lib.sf_last_error()
