"""GPU suite for ``syncfusion_amd.GraphedOnsetTrainStep``: the onset training step (forward, device loss and metrics, backward, and the HIP
AdamW when it is handed in) captured once and replayed.  A replay must be the eager ``loss="hip"`` step bit for bit, constructing the object
must not train the model, and the inference engine must follow the replayed updates.  (2, 3, 4, 32, 32) batches; every graphed object is
built on a fresh model, before any eager backward on it."""
from __future__ import annotations

import pytest
import torch
import torch.distributed as dist
import torch.nn as nn

from helpers import rel_l2
from test_gpu_onset_train import ONSET_FP32_TOL, _batch, _seeded_net

pytestmark = pytest.mark.gpu


def _model(cuda, seed: int = 7, **kw):
    from syncfusion_amd import OnsetModel

    net = _seeded_net(seed).to(cuda).train()
    return OnsetModel(1e-3, 0.9, 0.999, 1e-8, 1e-2, net, loss="hip", **kw).to(cuda)


def _state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


@pytest.mark.autograd
def test_construction_leaves_the_model_untouched(cuda):
    from syncfusion_amd import GraphedOnsetTrainStep

    model = _model(cuda)
    opt = model.configure_optimizers()
    before = _state(model)
    gs = GraphedOnsetTrainStep(model, _batch(2, 4, 32, 32, 21, cuda))
    torch.cuda.synchronize()
    after = model.state_dict()
    changed = [k for k in before if not torch.equal(before[k], after[k])]
    assert not changed, f"constructing the graphed step changed {changed[:5]}"
    assert int(model.model.net.model.stem[1].num_batches_tracked) == 0
    assert gs.metrics.shape == (3,) and gs.metrics.dtype == torch.float64 and gs.loss.shape == ()
    del opt


@pytest.mark.autograd
def test_one_replay_is_the_eager_step(cuda):
    from syncfusion_amd import GraphedOnsetTrainStep

    a, b = _model(cuda), _model(cuda)
    gs = GraphedOnsetTrainStep(a, _batch(2, 4, 32, 32, 21, cuda))
    batch = _batch(2, 4, 32, 32, 33, cuda)             # not the example batch: the copy-in is part of the step
    loss_g = gs.step(batch)
    loss_e = b.training_step(batch, 0)
    loss_e.backward()
    torch.cuda.synchronize()
    assert torch.equal(loss_g, loss_e.detach()), (float(loss_g), float(loss_e))
    assert torch.equal(gs.metrics, b.loss.last_metrics), (gs.metrics.tolist(), b.loss.last_metrics.tolist())
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    diff = [k for k in pa if pa[k].grad is None or not torch.equal(pa[k].grad, pb[k].grad)]
    assert not diff, f"gradients of the replay differ from the eager step: {diff[:5]}"
    ba, bb = dict(a.named_buffers()), dict(b.named_buffers())
    diff = [k for k in ba if not torch.equal(ba[k], bb[k])]
    assert not diff, f"running buffers of the replay differ from the eager step: {diff[:5]}"
    assert int(a.model.net.model.stem[1].num_batches_tracked) == 1


@pytest.mark.autograd
def test_three_replays_with_captured_adamw(cuda):
    from oracle import onsetnet_ref
    from syncfusion_amd import GraphedOnsetTrainStep
    from syncfusion_amd.optim import AdamW

    a, b = _model(cuda, optimizer="hip"), _model(cuda, optimizer="hip")
    x = torch.randn(2, 3, 4, 32, 32, generator=torch.Generator().manual_seed(8))
    with torch.no_grad():
        first = a.model.eval()(x.to(cuda)).cpu()        # builds the inference engine on the initial weights
    a.model.train()
    oa, ob = a.configure_optimizers(), b.configure_optimizers()
    assert isinstance(oa, AdamW)
    oa.max_grad_norm = ob.max_grad_norm = 0.5
    gs = GraphedOnsetTrainStep(a, _batch(2, 4, 32, 32, 21, cuda), optimizer=oa)
    assert not oa.state or all(float(st["step"]) == 0 for st in oa.state.values())     # the warm-up step was put back
    for i in range(3):
        batch = _batch(2, 4, 32, 32, 40 + 2 * i, cuda)
        gs.step(batch)
        ob.zero_grad(set_to_none=True)
        b.training_step(batch, i).backward()
        ob.step()
    torch.cuda.synchronize()
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    diff = [k for k in pa if not torch.equal(pa[k], pb[k])]
    assert not diff, f"parameters after three replays differ from three eager steps: {diff[:5]}"
    for k in pa:
        sa, sb = oa.state[pa[k]], ob.state[pb[k]]
        assert float(sa["step"]) == 3.0 == float(sb["step"]), k
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), f"moments of {k} differ"
    assert torch.equal(oa.last_grad_norm, ob.last_grad_norm)
    # the replays advanced the version counters of what they wrote: eval() rebuilds the engine on the updated weights and statistics
    with torch.no_grad():
        y = a.model.eval()(x.to(cuda)).cpu()
        ref = onsetnet_ref.onsetnet_forward({k: v.detach().float().cpu() for k, v in a.model.state_dict().items()}, x)
    e = rel_l2(y, ref)
    print(f"eval engine after 3 replayed steps: rel-L2 {e:.2e} (moved {rel_l2(first, ref):.2e} from the initial logits)")
    assert int(a.model.net.model.stem[1].num_batches_tracked) == 3
    assert rel_l2(first, ref) > 10 * ONSET_FP32_TOL, "the steps did not change the logits"
    assert e < ONSET_FP32_TOL


def test_refusals(cuda, tmp_path):
    from syncfusion_amd import GraphedOnsetTrainStep, OnsetModel

    batch = _batch(2, 4, 32, 32, 21, cuda)
    torch_loss = OnsetModel(1e-3, 0.9, 0.999, 1e-8, 1e-2, _seeded_net(7).to(cuda).train()).to(cuda)
    with pytest.raises(ValueError, match='loss="hip"'):
        GraphedOnsetTrainStep(torch_loss, batch)
    model = _model(cuda)
    with pytest.raises(TypeError, match="syncfusion_amd.optim.AdamW"):
        GraphedOnsetTrainStep(model, batch, optimizer=torch.optim.AdamW(model.parameters(), fused=True))
    sync = nn.SyncBatchNorm.convert_sync_batchnorm(_model(cuda))
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        with pytest.raises(RuntimeError, match="synchronised BatchNorm cannot be captured"):
            GraphedOnsetTrainStep(sync, batch)
    finally:
        dist.destroy_process_group()
    model.model.eval()
    with pytest.raises(RuntimeError, match="eval mode"):
        GraphedOnsetTrainStep(model, batch)
    for m in (torch_loss, model, sync):      # nothing ran: no running statistic moved
        assert int(m.model.net.model.stem[1].num_batches_tracked) == 0
