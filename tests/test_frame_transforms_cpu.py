"""Host side of the onset data's training transforms (syncfusion_amd/frame_transforms.py): constructor semantics, the random
parameters and the order in which they consume a generator, ``Compose``'s shape validation, the ``class_path`` loader, and the fixture
conditions of the GPU tests checked with the oracle alone.  Nothing here needs a GPU."""
import inspect
import os

import pytest
import torch
import yaml

import frames_augment_ref as R
from syncfusion_amd import config
from syncfusion_amd import frame_transforms as ft
from syncfusion_amd._lib import SyncFusionAmdError

NORM = dict(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
REFERENCE_YAML = "/root/reference/cfg/data/data-onset-greatesthit-augment.yaml"


def _full(size=128):
    return ft.Compose([ft.Resize(size, antialias=True), ft.RandomCrop(112), ft.ColorJitter(0.4, 0.2, 0.4, 0.1), ft.Normalize(**NORM)])


def test_constructor_ranges_and_errors():
    j = ft.ColorJitter(brightness=0.4, contrast=0.2, saturation=0.4, hue=0.1)
    assert j.brightness == pytest.approx((0.6, 1.4)) and j.contrast == pytest.approx((0.8, 1.2)) and j.hue == pytest.approx((-0.1, 0.1))
    assert ft.ColorJitter(brightness=1.5).brightness == (0.0, 2.5)                # floor max(0, 1 - v)
    assert ft.ColorJitter(brightness=(0.5, 0.7)).brightness == (0.5, 0.7)
    z = ft.ColorJitter(0.1, 0.1, 0, 0)                                            # main/datamodule_onset.py's variant: absent, not neutral
    assert z.saturation is None and z.hue is None and z.brightness is not None
    assert ft.ColorJitter().ranges() == [None] * 4
    for bad in (dict(brightness=-0.1), dict(hue=0.6), dict(hue=(-0.6, 0.1)), dict(contrast=(1.2, 0.8)), dict(saturation=(-1, 1)),
                dict(brightness=float("nan"))):
        with pytest.raises(ValueError):
            ft.ColorJitter(**bad)
    with pytest.raises(TypeError):
        ft.ColorJitter(brightness="0.4")
    assert ft.Resize(128).size == 128 and ft.Resize([128]).size == 128 and ft.Resize((112, 112)).size == (112, 112)
    assert ft.Resize(128).output_size((240, 320)) == (128, 170)                   # int(128 * 320 / 240)
    assert ft.Resize(128).output_size((320, 240)) == (170, 128)
    assert ft.Resize(128).output_size((130, 100)) == (166, 128)
    assert ft.Resize((112, 112)).output_size((240, 320)) == (112, 112)
    assert ft.RandomCrop(112).size == (112, 112) and ft.CenterCrop((100, 90)).size == (100, 90)
    with pytest.raises(TypeError):
        ft.Resize("128")
    with pytest.raises(ValueError):
        ft.Resize(0)
    with pytest.raises(ValueError):
        ft.RandomCrop((1, 2, 3))
    with pytest.raises(ValueError):
        ft.Normalize([0.5, 0.5, 0.5], [0.2, 0.0, 0.2])
    with pytest.raises(ValueError):
        ft.Normalize([0.5], [0.2])


def test_sample_ranges_orders_and_seed():
    chain = _full()
    p = chain.sample(1000, (240, 320), torch.Generator().manual_seed(0))
    assert p.resized_hw == (128, 170) and p.out_hw == (112, 112) and len(p) == 1000
    assert 0 <= int(p.top.min()) and int(p.top.max()) <= 16 and 0 <= int(p.left.min()) and int(p.left.max()) <= 58
    assert int(p.top.max()) == 16 and int(p.left.max()) == 58 and int(p.top.min()) == 0 and int(p.left.min()) == 0   # both ends occur
    for i, (lo, hi) in enumerate([(0.6, 1.4), (0.8, 1.2), (0.6, 1.4), (-0.1, 0.1)]):
        col = p.factor[:, i].double()
        assert lo - 1e-6 <= float(col.min()) and float(col.max()) <= hi + 1e-6 and float(col.max() - col.min()) > 0.9 * (hi - lo)
    assert all(sorted(o) == [0, 1, 2, 3] for o in p.order.tolist())
    assert len({tuple(o) for o in p.order.tolist()}) == 24
    assert p.mask.tolist() == [15] * 1000
    q = chain.sample(1000, (240, 320), torch.Generator().manual_seed(0))
    assert torch.equal(p.table(), q.table())
    assert not torch.equal(p.table(), chain.sample(1000, (240, 320), torch.Generator().manual_seed(1)).table())
    t = p.table()
    assert t.shape == (1000, 12) and t.dtype == torch.int32 and torch.equal(t[:, 6:10].contiguous().view(torch.float32), p.factor)
    assert torch.equal(t[:, 0], p.top) and torch.equal(t[:, 2:6], p.order) and torch.equal(t[:, 10], p.mask) and int(t[:, 11].abs().max()) == 0


def test_sample_follows_torchvisions_order_of_consumption():
    """RandomCrop.get_params: randint(0, rh - th + 1), randint(0, rw - tw + 1); ColorJitter.get_params: randperm(4), then uniform_ for
    brightness, contrast, saturation, hue, skipping absent ones -- clip after clip."""
    g, h = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    chain = ft.Compose([ft.Resize(128, antialias=True), ft.RandomCrop(112), ft.ColorJitter(0.1, 0.1, 0, 0.05), ft.Normalize(**NORM)])
    p = chain.sample(3, (240, 320), g)
    for k in range(3):
        assert int(p.top[k]) == int(torch.randint(0, 128 - 112 + 1, size=(1,), generator=h))
        assert int(p.left[k]) == int(torch.randint(0, 170 - 112 + 1, size=(1,), generator=h))
        assert p.order[k].tolist() == torch.randperm(4, generator=h).tolist()
        assert float(p.factor[k, 0]) == float(torch.empty(1).uniform_(0.9, 1.1, generator=h))
        assert float(p.factor[k, 1]) == float(torch.empty(1).uniform_(0.9, 1.1, generator=h))
        assert float(p.factor[k, 2]) == 1.0                                       # absent: no draw, neutral placeholder, mask bit clear
        assert float(p.factor[k, 3]) == float(torch.empty(1).uniform_(-0.05, 0.05, generator=h))
    assert p.mask.tolist() == [0b1011] * 3
    assert torch.equal(g.get_state(), h.get_state())


def test_absent_operations_and_whole_frame_crops_consume_nothing():
    # a jitter whose operations are all absent still draws its permutation (torchvision does), but no factor
    a, b = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    ft.Compose([ft.Resize(128, antialias=True), ft.RandomCrop(112), ft.ColorJitter(0.4, 0, 0, 0.1), ft.Normalize(**NORM)]).sample(4, (240, 320), a)
    for _ in range(4):
        torch.randint(0, 17, size=(1,), generator=b), torch.randint(0, 59, size=(1,), generator=b), torch.randperm(4, generator=b)
        torch.empty(1).uniform_(0.6, 1.4, generator=b), torch.empty(1).uniform_(-0.1, 0.1, generator=b)
    assert torch.equal(a.get_state(), b.get_state())
    # no ColorJitter, crop == resized frame: the generator is untouched
    c = torch.Generator().manual_seed(9)
    before = c.get_state().clone()
    p = ft.Compose([ft.Resize(112, antialias=True), ft.RandomCrop(112), ft.Normalize(**NORM)]).sample(3, (112, 112), c)
    assert torch.equal(c.get_state(), before) and p.top.tolist() == [0, 0, 0] and p.mask.tolist() == [0, 0, 0]
    # CenterCrop: torchvision's int(round((rh - th) / 2.0)), no draw
    p = ft.Compose([ft.Resize(128, antialias=True), ft.CenterCrop(112), ft.Normalize(**NORM)]).sample(2, (240, 320), c)
    assert torch.equal(c.get_state(), before) and p.top.tolist() == [8, 8] and p.left.tolist() == [29, 29]
    with pytest.raises(SyncFusionAmdError, match="larger than the resized frame"):
        ft.Compose([ft.Resize(64, antialias=True), ft.RandomCrop(112), ft.Normalize(**NORM)]).sample(1, (240, 320), c)


def test_compose_names_the_offending_entry():
    n = ft.Normalize(**NORM)
    r = ft.Resize(128, antialias=True)
    ft.Compose([ft.Resize((112, 112), antialias=True), n])                        # the bare evaluation chain
    ft.Compose([r, ft.CenterCrop(112), n])
    ft.Compose([r, ft.ColorJitter(0.1), n])
    for bad, text in [([ft.Resize(128, antialias=False), n], r"entry 0 .*antialias=True"),
                      ([ft.Resize(128), n], r"entry 0 .*antialias=True"),
                      ([ft.Resize(128, max_size=200, antialias=True), n], r"entry 0 .*max_size"),
                      ([ft.Resize(128, interpolation="nearest", antialias=True), n], r"entry 0 .*bilinear"),
                      ([r, ft.RandomCrop(112, padding=4), n], r"entry 1 .*padding"),
                      ([r, ft.RandomCrop(112, pad_if_needed=True), n], r"entry 1 .*padding"),
                      ([ft.RandomCrop(112), r, n], r"entry 0 .*must be a Resize"),
                      ([r, ft.ColorJitter(0.1), ft.RandomCrop(112), n], r"entry 2 .*out of place"),
                      ([r, ft.RandomCrop(112), ft.CenterCrop(112), n], r"entry 2 .*out of place"),
                      ([r, n, ft.ColorJitter(0.1)], r"entry 2 .*out of place"),
                      ([r, ft.RandomCrop(112)], r"must end with a Normalize"),
                      ([r, torch.nn.Identity(), n], r"entry 1 .*not one of"),
                      ([], r"empty")]:
        with pytest.raises(SyncFusionAmdError, match=text):
            ft.Compose(bad)
    with pytest.raises(SyncFusionAmdError, match="no CPU execution path"):
        _full()(torch.zeros(1, 2, 240, 320, 3, dtype=torch.uint8))


YAML_LITERAL = """
train_frames_transforms:
  class_path: torchvision.transforms.Compose
  init_args:
    transforms:
    - class_path: torchvision.transforms.Resize
      init_args:
        size: 128
        antialias: True
    - class_path: torchvision.transforms.RandomCrop
      init_args:
        size: 112
    - class_path: torchvision.transforms.ColorJitter
      init_args:
        brightness: 0.4
        contrast: 0.2
        saturation: 0.4
        hue: 0.1
    - class_path: torchvision.transforms.Normalize
      init_args:
        mean: [0.485, 0.456, 0.406]
        std: [0.229, 0.224, 0.225]
test_frames_transforms: null
"""


def _is_training_chain(c):
    assert isinstance(c, ft.Compose) and c.resize.size == 128 and c.resize.antialias is True
    assert isinstance(c.crop, ft.RandomCrop) and c.crop.size == (112, 112)
    assert c.jitter.brightness == pytest.approx((0.6, 1.4)) and c.jitter.contrast == pytest.approx((0.8, 1.2))
    assert c.jitter.saturation == pytest.approx((0.6, 1.4)) and c.jitter.hue == pytest.approx((-0.1, 0.1))
    assert c.normalize.mean == (0.485, 0.456, 0.406) and c.normalize.std == (0.229, 0.224, 0.225)


def _is_default_chain(c):
    assert isinstance(c, ft.Compose) and c.resize.size == (112, 112) and c.crop is None and c.jitter is None
    assert c.normalize.mean == (0.485, 0.456, 0.406) and c.normalize.std == (0.229, 0.224, 0.225)


def test_class_path_loader_on_a_yaml_literal():
    cfg = yaml.safe_load(YAML_LITERAL)
    _is_training_chain(config.instantiate_frames_transforms(cfg["train_frames_transforms"]))
    _is_default_chain(config.instantiate_frames_transforms(cfg["test_frames_transforms"]))
    _is_training_chain(config.instantiate_class(cfg)["train_frames_transforms"])
    with pytest.raises(ValueError, match="unexpected keys"):
        config.instantiate_class({"class_path": "torchvision.transforms.CenterCrop", "init_args": {"size": 112}, "size": 112})
    with pytest.raises(SyncFusionAmdError, match="entry 0"):
        config.instantiate_class({"class_path": "torchvision.transforms.Compose", "init_args": {"transforms": [
            {"class_path": "torchvision.transforms.Resize", "init_args": {"size": 128}},
            {"class_path": "torchvision.transforms.Normalize", "init_args": {"mean": [0.5, 0.5, 0.5], "std": [0.2, 0.2, 0.2]}}]}})


@pytest.mark.skipif(not os.path.exists(REFERENCE_YAML), reason="the reference tree is not on this machine")
def test_class_path_loader_on_the_reference_file():
    args = config.load_yaml(REFERENCE_YAML)["data"]["init_args"]
    _is_training_chain(config.instantiate_frames_transforms(args["train_frames_transforms"]))
    _is_training_chain(config.instantiate_frames_transforms(args["val_frames_transforms"]))
    _is_default_chain(config.instantiate_frames_transforms(args["test_frames_transforms"]))


def test_chunk_entry_points_keep_their_arguments():
    from syncfusion_amd import video_chunks as vc

    p = list(inspect.signature(vc.chunk_clip).parameters.values())
    assert [q.name for q in p[:4]] == ["chunk", "device", "frame_file_suffix", "size"]
    assert p[2].default == ".jpg" and p[3].default == (112, 112)
    assert {q.name: q.default for q in p[4:]} == {"frames_transforms": None, "generator": None}
    p = list(inspect.signature(vc.iter_clips).parameters.values())
    assert [q.name for q in p[:4]] == ["chunks", "batch_size", "device", "frame_file_suffix"] and p[3].default == ".jpg"
    assert {q.name: q.default for q in p[4:]} == {"frames_transforms": None, "shuffle": False, "drop_last": False, "generator": None}


def test_package_exports_and_symbols():
    import syncfusion_amd as sa
    from syncfusion_amd import _lib

    assert sa.frame_transforms is ft and "frame_transforms" in sa.__all__
    assert "sf_frames_augment" in _lib.SYMBOLS and "sf_frames_augment_workspace_bytes" in _lib.SYMBOLS
    lib = _lib.load()
    assert lib.sf_frames_augment_workspace_bytes(16, 30, 112, 112) == 16 * 30 * 49 * 4
    # the host-side validation needs no device: a bad table is refused before any HIP call
    tab = _full().sample(2, (240, 320), torch.Generator().manual_seed(0))
    tab.order[1, 0] = tab.order[1, 1]
    host = tab.table()
    rc = lib.sf_frames_augment(host.data_ptr(), 2, 2, 240, 320, 128, 170, 112, 112, host.data_ptr(), host.data_ptr(), None, None, host.data_ptr(),
                               None, 0, None)
    assert rc != 0                                                                # (null mean / std: refused as a bad argument, nothing touched)
    import ctypes as C

    m, s = (C.c_float * 3)(0.485, 0.456, 0.406), (C.c_float * 3)(0.229, 0.224, 0.225)
    rc = lib.sf_frames_augment(host.data_ptr(), 2, 2, 240, 320, 128, 170, 112, 112, host.data_ptr(), host.data_ptr(), m, s, host.data_ptr(), None, 0, None)
    assert rc != 0 and b"not a permutation" in lib.sf_last_error()


def test_fixture_frames_meet_the_conditions_of_the_gpu_tests():
    """with the oracle alone: every hue sector holds >= 1 % of the pixels entering the hue step, and >= 0.5 % of the values reach each
    clamp bound under strong brightness and strong contrast -- for every geometry the GPU tests use"""
    for (N, T, H, W), size in [((2, 4, 240, 320), 128), ((1, 4, 320, 240), 128), ((3, 5, 130, 100), 128), ((1, 3, 112, 112), 112)]:
        u8 = R.make_frames(N, T, H, W, seed=H)
        chain = _full(size)
        for op, f in [(0, 1.4), (1, 1.2), (3, 0.1), (3, -0.1)]:
            p = chain.sample(N, (H, W), torch.Generator().manual_seed(4))
            p.mask[:] = 1 << op
            p.factor[:, op] = f
            probe = {}
            out = R.transform_batch(u8, p, dtype=torch.float64, probe=probe)
            assert out.shape == (N, 3, T, 112, 112)
            if op == 3:
                s = torch.cat([v.flatten() for v in probe["hue_sector"]])
                assert min(float((s == k).double().mean()) for k in range(6)) >= 0.01
            else:
                v = torch.cat([x.flatten() for x in probe["preclamp_" + ft.OPS[op]]])
                assert float((v <= 0).double().mean()) >= 0.005 and float((v >= 1).double().mean()) >= 0.005


def test_oracle_resize_and_crop_is_a_slice_of_the_pinned_transform():
    """the PINNED half: with no crop offset and no colour operation the oracle is oracle/frames_ref.py (ATen's antialiased kernel)"""
    from oracle import frames_ref

    u8 = R.make_frames(1, 2, 240, 320, seed=2)
    chain = ft.Compose([ft.Resize((112, 112), antialias=True), ft.Normalize(**NORM)])
    p = chain.sample(1, (240, 320))
    assert torch.equal(R.transform_batch(u8, p, dtype=torch.float32), frames_ref.frames_transform(u8))


def test_oracle_matches_torchvision():
    """The pin of the UNPINNED half: the restated colour operations and the RNG consumption order against torchvision itself, the day it
    is installed (it is absent where this was written)."""
    tv = pytest.importorskip("torchvision")
    from torchvision import transforms as T

    from syncfusion_amd import frame_transforms as ft

    u8 = R.make_frames(3, 4, 240, 320, seed=5)
    ours = _full()
    theirs = T.Compose([T.Resize(128, antialias=True), T.RandomCrop(112), T.ColorJitter(0.4, 0.2, 0.4, 0.1),
                        T.Normalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])])
    params = ours.sample(3, (240, 320), torch.Generator().manual_seed(77))
    want = R.transform_batch(u8, params, dtype=torch.float32)
    torch.manual_seed(77)          # torchvision draws from the global generator, clip after clip
    got = torch.stack([theirs(u8[n].permute(0, 3, 1, 2).float() / 255.0).permute(1, 0, 2, 3) for n in range(3)])
    assert tv is not None and isinstance(ours, ft.Compose)
    assert float((got - want).abs().max()) <= 1e-6
