"""The U-Net engine's launch sequence, pinned per shape (MI355X).

Which chain an item group runs on -- thin, thin with the fused tail, wide (with Modulation's LayerNorm folded or not), channel-block,
direct channel-block -- and whether the attention pre-norm is folded is decided on the host (unet_engine.cpp, item_plan).  Parity tests see
a wrong decision only as a slightly different error; this file compares, for every case below, the whole profiled evaluation with
tests/golden/unet_launches.npz: the label, U-Net depth, algorithmic flops and algorithmic bytes of every launch, in order, and launch_count().
Flops and bytes are doubles computed on the host from the shapes, so they are compared with ==.

The fixture was recorded by tools/record_unet_launches.py from the library as it stood BEFORE the item path was rebuilt around one plan per
item (item_plan) and one function per chain.  It is re-recorded only by a change that means to move a launch, and that change says so.

Cases (one evaluation each; the launch sequence is a function of the shapes alone, so the inputs are constants):
  small net (helpers.SMALL_UNET), four engines, (B, L0) = (1, 16), (3, 112), (2, 1024): thin levels with and without attention, a single
      position at the deepest level, the depth-0 vector kernels; one transposed-upsample small net;
  full model, L0 = 45056, four engines, B = 1, 2, 8, 16, 32 and B = 8 guided: one and two branches, the direct channel-block chain (up to its
      2816-row cap), the channel-block chain, the wide chain with and without the folded Modulation;
  full model, (B, L0) = (1, 1024): one position at the deepest level.
"""
import os

import numpy as np
import pytest
import torch

from helpers import reference_model_config, small_unet_module

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet_launches.npz")
ENGINES = ("fp32", "fp32x", "bf16", "fp16")
# every kernel family of the item path must be reached by some case (checked on the fixture, so a re-recording cannot lose one silently)
MUST_REACH = ("conv_thin", "conv_cb", "conv_cb_gn", "conv_cb_ln", "cb_reduce_gn", "cb_reduce_ln", "gn_silu", "gn_stats", "ln_modulate", "attention")


def cases():
    """(net, engine, B, L0, embedding_scale), engine-major per net so that a net's engine is repacked once per arithmetic type"""
    out = []
    for dtype in ENGINES:
        out += [("small", dtype, B, L0, 1.0) for B, L0 in ((1, 16), (3, 112), (2, 1024))]
    out.append(("small_transposed", "bf16", 3, 112, 1.0))
    for dtype in ENGINES:
        out += [("full", dtype, B, 45056, 1.0) for B in (1, 2, 8, 16, 32)]
        out.append(("full", dtype, 8, 45056, 2.0))
        out.append(("full", dtype, 1, 1024, 1.0))
    return out


def case_id(case):
    net, dtype, B, L0, scale = case
    return f"{net}-{dtype}-B{B}-L{L0}" + ("-guided" if scale != 1.0 else "")


class Nets:
    """the three networks, built on first use and kept for the module"""

    def __init__(self, device):
        self.device, self.nets = device, {}

    def get(self, name):
        if name not in self.nets:
            if name == "full":     # as test_gpu_models.full_model
                import syncfusion_amd as sa

                torch.manual_seed(1234)
                net = sa.instantiate(reference_model_config()).model.net
            else:
                net = small_unet_module(upsample_mode="transpose" if name == "small_transposed" else "nearest")
            self.nets[name] = net.to(self.device)
        return self.nets[name]


def run_case(nets, case):
    """-> (labels, depths, flops, bytes, launch_count) of one profiled evaluation"""
    name, dtype, B, L0, scale = case
    net = nets.get(name)
    hp, dev = net.hparams, nets.device
    x = torch.zeros(B, hp["in_channels"], L0, device=dev)
    sigma = torch.full((B,), 0.5, device=dev)
    emb = torch.zeros(B, hp["embedding_max_length"], hp["embedding_features"], device=dev)
    emb[..., 0] = 1.0
    chans, L = [], L0
    for d, c in enumerate(hp["context_channels"]):
        L //= hp["factors"][d]
        chans.append(torch.zeros(B, c, L, device=dev))
    prev, net.compute_dtype = net.compute_dtype, dtype
    try:
        with torch.no_grad():
            recs = net.engine().profile_forward(x, sigma, chans, emb, scale, with_depth=True)
            count = net.engine().launch_count()
    finally:
        net.compute_dtype = prev
    return [r[0] for r in recs], [r[4] for r in recs], [r[2] for r in recs], [r[3] for r in recs], count


def pack(results):
    """{case id: run_case result} -> the arrays of the .npz: the distinct labels once, the launches of all cases end to end"""
    strings = sorted({s for labels, *_ in results.values() for s in labels})
    index = {s: i for i, s in enumerate(strings)}
    ids = list(results)
    return {
        "strings": np.asarray(strings),
        "cases": np.asarray(ids),
        "start": np.cumsum([0] + [len(results[k][0]) for k in ids]).astype(np.int64),
        "label": np.asarray([index[s] for k in ids for s in results[k][0]], dtype=np.int16),
        "depth": np.asarray([d for k in ids for d in results[k][1]], dtype=np.int8),
        "flops": np.asarray([f for k in ids for f in results[k][2]], dtype=np.float64),
        "bytes": np.asarray([b for k in ids for b in results[k][3]], dtype=np.float64),
        "launch_count": np.asarray([results[k][4] for k in ids], dtype=np.int32),
    }


@pytest.fixture(scope="module")
def pinned():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def nets(cuda):
    return Nets(cuda)


@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_every_launch_is_what_the_fixture_pins(nets, pinned, case):
    ids = [str(s) for s in pinned["cases"]]
    assert case_id(case) in ids, "the case list changed: the fixture no longer lines up with it"
    i = ids.index(case_id(case))
    a, b = int(pinned["start"][i]), int(pinned["start"][i + 1])
    strings = pinned["strings"]
    want = [(str(strings[j]), int(d), float(f), float(y)) for j, d, f, y in
            zip(pinned["label"][a:b], pinned["depth"][a:b], pinned["flops"][a:b], pinned["bytes"][a:b])]
    labels, depths, flops, nbytes, count = run_case(nets, case)
    have = list(zip(labels, depths, flops, nbytes))
    bad = [(k, h, w) for k, (h, w) in enumerate(zip(have, want)) if h != w]
    print(f"{case_id(case)}: {len(have)} launches (pinned {len(want)}), launch_count {count} (pinned {int(pinned['launch_count'][i])})")
    assert len(have) == len(want) and not bad, (
        f"{case_id(case)}: {len(have)} launches now, {len(want)} pinned; first differences (index: now / pinned):\n" +
        "\n".join(f"  {k}: {h} / {w}" for k, h, w in bad[:8]))
    assert count == int(pinned["launch_count"][i])


def test_the_fixture_holds_exactly_these_cases(pinned):
    assert [str(s) for s in pinned["cases"]] == [case_id(c) for c in cases()]
    assert len(pinned["start"]) == len(pinned["cases"]) + 1 and int(pinned["start"][-1]) == len(pinned["label"])


def test_the_fixture_reaches_every_chain(pinned):
    strings = {str(s) for s in pinned["strings"][np.unique(pinned["label"])]}
    missing = [s for s in MUST_REACH if s not in strings]
    assert not missing, f"no case reaches {missing}"
    # A LayerNorm-folded GEMM carries the label of the plain one; it shows as the launch it removes.  The launch in front of "attention" is
    # the qkv projection: with the pre-norm folded no ln_modulate stands in front of that, otherwise one does -- both endings must occur.
    names = [str(s) for s in pinned["strings"][pinned["label"]]]
    before_qkv = {names[k - 2] == "ln_modulate" for k, s in enumerate(names) if s == "attention"}
    assert before_qkv == {True, False}, "the cases must reach the qkv projection with and without the folded pre-norm"
