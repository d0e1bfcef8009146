"""The GEMM descriptions of the two CLAP engines, pinned byte for byte (host only).

``sf_clap_audio_describe`` and ``sf_clap_text_describe`` print, per Linear of the network, its shape and the kernel the dispatcher gives
it.  Which kernel that is depends on fields of the argument block that look harmless (``solo``, ``Lout``, ``Lsrc``); a builder that fills
one of them differently moves a launch to another family, and parity tests see that only as a slightly different error.  This file compares
the full text of every case below, and the code and message of every refusal, with tests/golden/engine_describe.json.

The fixture was recorded by running this file as a script (``SF_LIB_PATH=<library> python tests/test_engine_describe.py``) against the
library as it stood BEFORE the engines' host glue moved into engine_common (one guard, one set of ConvGemmArgs builders, one description
writer).  It is re-recorded only by a change that means to move a launch or to change a message, and that change says so.

Cases:
  audio  the default ClapAudioConfig and the smallest the config checks admit (one stage of one block, embed_dim 32, spec_size 32, one
         head), each at B = 1 and 4;
  text   the default ClapTextConfig and a reduced one (one layer, hidden 64, one head, intermediate 64), each at (B, S) = (1, 1), (1, 77)
         and (16, 16);
  so M = 1 rows and the narrowest K and N are there, where the choice between the small-tile families and the classic tile is most
  sensitive;
  refusals: a text buffer too small, B = 0, S = 0, S above max_length, S above what the kernels take, a null buffer.
"""
import ctypes as C
import json
import os
import types
from dataclasses import replace

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_describe.json")
AUDIO_CONFIGS = {"default": {}, "reduced": dict(spec_size=32, embed_dim=32, depths=(1,), num_heads=(1,))}
TEXT_CONFIGS = {"default": {}, "reduced": dict(layers=1, hidden=64, heads=1, intermediate=64)}
AUDIO_BATCHES = (1, 4)
TEXT_SHAPES = ((1, 1), (1, 77), (16, 16))


def audio_config(name):
    from syncfusion_amd.clap import ClapAudioConfig, ClapAudioEmbedder

    cfg = replace(ClapAudioConfig(), **AUDIO_CONFIGS[name])      # the engine's own checks (check_config) are what describe runs
    return ClapAudioEmbedder.engine_config(types.SimpleNamespace(config=cfg))      # the method reads the configuration only


def text_config(name):
    from syncfusion_amd.clap_text import ClapEmbedder, ClapTextConfig

    cfg = replace(ClapTextConfig(), **TEXT_CONFIGS[name])
    return ClapEmbedder.text_engine_config(types.SimpleNamespace(text_config=cfg))


def describe(entry, cfg, dims, capacity=1 << 14, null=False):
    """(code, text on success / the library's message on a refusal)"""
    from syncfusion_amd import _lib

    lib = _lib.load()
    buf = C.create_string_buffer(max(capacity, 1))
    code = getattr(lib, entry)(C.byref(cfg), *dims, None if null else buf, capacity)
    return [code, buf.value.decode() if code == 0 else lib.sf_last_error().decode()]


def observed():
    out = {}
    for name in AUDIO_CONFIGS:
        for B in AUDIO_BATCHES:
            out[f"audio/{name}/B{B}"] = describe("sf_clap_audio_describe", audio_config(name), (B,))
    for name in TEXT_CONFIGS:
        for B, S in TEXT_SHAPES:
            out[f"text/{name}/B{B}-S{S}"] = describe("sf_clap_text_describe", text_config(name), (B, S))
    a, t = audio_config("default"), text_config("default")
    out["audio/refusal/capacity"] = describe("sf_clap_audio_describe", a, (1,), capacity=8)
    out["audio/refusal/B0"] = describe("sf_clap_audio_describe", a, (0,))
    out["audio/refusal/null"] = describe("sf_clap_audio_describe", a, (1,), null=True)
    out["text/refusal/capacity"] = describe("sf_clap_text_describe", t, (1, 4), capacity=8)
    out["text/refusal/B0"] = describe("sf_clap_text_describe", t, (0, 4))
    out["text/refusal/S0"] = describe("sf_clap_text_describe", t, (1, 0))
    out["text/refusal/S-above-max_length"] = describe("sf_clap_text_describe", t, (1, 78))
    out["text/refusal/S-above-the-kernels"] = describe("sf_clap_text_describe", t, (1, 200))
    out["text/refusal/null"] = describe("sf_clap_text_describe", t, (1, 4), null=True)
    return out


def test_describe_text_and_refusals_match_the_fixture():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = observed()
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key
    # the fixture itself: every description is a success without an invalid plan, every refusal keeps its code
    for key, (code, text) in want.items():
        if "/refusal/" not in key:
            assert code == 0 and text.endswith("\n") and "invalid" not in text, key
    codes = {key.split("/refusal/")[1]: want[key][0] for key in want if key.startswith("text/refusal/")}
    assert codes == {"capacity": 1, "B0": 1, "S0": 1, "S-above-max_length": 3, "S-above-the-kernels": 6, "null": 1}
    assert [want[f"audio/refusal/{k}"][0] for k in ("capacity", "B0", "null")] == [1, 1, 1]
    assert "(x 12 layers)" in want["text/default/B1-S1"][1] and "layers" not in want["audio/default/B1"][1]
    assert "M 1 N 192 K 64" in want["text/reduced/B1-S1"][1] and "M 64 N 96 K 32" in want["audio/reduced/B1"][1]


if __name__ == "__main__":      # re-record (module docstring)
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    recorded = observed()
    with open(FIXTURE, "w") as f:
        json.dump(recorded, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", FIXTURE)
