"""Inpainting sampler, host side: the numpy Philox restatement against its known answers, the oracle loop's identities, the window
and region helpers of the generation API, and the C header."""
import os

import numpy as np
import pytest
import torch

import inpaint_ref
from helpers import ROOT

from inpaint_ref import MEAN_GATE, STAT_N, STAT_SEED, VAR_GATE


def test_philox_known_answers():
    for counter, key, want in inpaint_ref.PHILOX_KAT:
        got = inpaint_ref.philox4x32_10([np.array([c], dtype=np.uint64) for c in counter], key)
        assert tuple(int(g[0]) for g in got) == want, [hex(int(g[0])) for g in got]


def test_philox_words_layout():
    """counter = (g lo, g hi, k, 0), key = (seed lo, seed hi); an offset draw is a slice of the larger one."""
    seed, k = (7 << 32) | 9, 5
    w = inpaint_ref.philox_words(seed, k, 0, 64)
    one = inpaint_ref.philox4x32_10([np.array([c], dtype=np.uint64) for c in (3, 0, k, 0)], (9, 7))
    assert [int(v) for v in w[3]] == [int(o[0]) for o in one]
    big = inpaint_ref.philox_normal(seed, k, 0, 4099)
    assert np.array_equal(inpaint_ref.philox_normal(seed, k, 1027, 1001), big[1027:2028])
    hi = inpaint_ref.philox_words(seed, k, (1 << 34) + 4, 4)       # group index above 2**32: its high word is in the counter
    want = inpaint_ref.philox4x32_10([np.array([c], dtype=np.uint64) for c in (1, 1, k, 0)], (9, 7))
    assert [int(v) for v in hi[0]] == [int(o[0]) for o in want]


def test_philox_normal_statistics_of_the_gpu_test_seed():
    z = inpaint_ref.philox_normal(STAT_SEED, 0, 0, STAT_N)
    assert np.isfinite(z).all() and np.abs(z).max() < 5.8
    assert abs(z.mean()) < MEAN_GATE and abs(z.var() - 1.0) < VAR_GATE, (z.mean(), z.var())


def _toy_net(x, sig):
    return 0.3 * torch.roll(x, 1, -1) - sig.reshape(-1, 1, 1) * torch.tanh(x)


def test_oracle_loop_reduces_to_vsampler():
    from oracle import sampler_ref

    g = torch.Generator().manual_seed(0)
    x0, src = torch.randn(2, 1, 64, generator=g), torch.randn(2, 1, 64, generator=g)
    mask = torch.zeros(2, 1, 64, dtype=torch.bool)
    out = inpaint_ref.vinpaint(_toy_net, src, mask, 7, 1, x0, lambda k: torch.randn(2, 1, 64, generator=g))
    assert torch.equal(out, sampler_ref.vsample(_toy_net, x0, 7))


def test_oracle_loop_full_mask_returns_source():
    g = torch.Generator().manual_seed(1)
    x0, src = torch.randn(2, 1, 64, generator=g), torch.randn(2, 1, 64, generator=g)
    mask = torch.ones(2, 1, 1, dtype=torch.bool)            # broadcast over the samples
    calls = []

    def noise(k):
        calls.append(k)
        return torch.randn(2, 1, 64, generator=g)

    out = inpaint_ref.vinpaint(_toy_net, src, mask, 4, 3, x0, noise)
    assert torch.equal(out, src)
    assert calls == list(range(12))


def test_long_windows():
    from syncfusion_amd import long_windows

    assert long_windows(704, 704, 96) == [(0, 0)]
    assert long_windows(705, 704, 96) == [(0, 0), (1, 703)]
    hop = 704 - 96
    assert long_windows(704 + 2 * hop, 704, 96) == [(0, 0), (hop, 96), (2 * hop, 96)]          # an exact multiple of the hop
    assert long_windows(2 * 704 - 100, 704, 96) == [(0, 0), (604, 100)]
    w = long_windows(5000, 704, 96)
    assert w[-1][0] == 5000 - 704 and all(k >= 96 for _, k in w[1:])
    covered = np.zeros(5000, dtype=bool)
    for s, _ in w:
        covered[s:s + 704] = True
    assert covered.all()
    for total, length, overlap in [(704, 704, 0), (704, 704, 704), (703, 704, 96), (704, 96, 100), (704, 704, -1)]:
        with pytest.raises(ValueError):
            long_windows(total, length, overlap)


def test_regions_to_keep_mask():
    from syncfusion_amd import regions_to_keep_mask

    m = regions_to_keep_mask([(3, 7), (7, 9), (20, 20)], 2, 32)          # touching ranges and an empty one
    assert m.shape == (2, 1, 32) and m.dtype == torch.bool
    want = torch.ones(32, dtype=torch.bool)
    want[3:9] = False
    assert torch.equal(m[0, 0], want) and torch.equal(m[1, 0], want)
    per = regions_to_keep_mask([[(0, 4)], []], 2, 32)                    # per clip; a clip without regions keeps everything
    assert not per[0, 0, :4].any() and per[0, 0, 4:].all() and per[1].all()
    assert regions_to_keep_mask([], 2, 32).all()
    assert not regions_to_keep_mask([(0, 32)], 1, 32).any()
    for bad in ([(5, 3)], [(-1, 3)], [(0, 33)], [[(0, 1)]], [(1, 2, 3)]):
        with pytest.raises(ValueError):
            regions_to_keep_mask(bad, 2, 32)


def test_inpaint_batch_wants_exactly_one_of_regions_and_mask():
    from syncfusion_amd import inpaint_batch

    a = torch.zeros(1, 1, 32)
    with pytest.raises(ValueError, match="exactly one"):
        inpaint_batch(None, a, a)
    with pytest.raises(ValueError, match="exactly one"):
        inpaint_batch(None, a, a, regions=[(0, 4)], keep_mask=torch.ones(1, 1, 32, dtype=torch.bool))


def test_header_declares_the_new_symbols():
    from syncfusion_amd import _lib

    text = open(os.path.join(ROOT, "include", "syncfusion_amd.h")).read()
    for name in ("sf_vinpaint", "sf_vinpaint_workspace_bytes", "sf_op_philox_normal", "sf_op_vinpaint_update"):
        assert f" {name}(" in text, name
        assert name in _lib.SYMBOLS
