"""Milliseconds per text-embedding call of ``ClapEmbedder`` (HIP; the full RoBERTa-base text branch, seeded weights) for 1, 8 and 16 prompts:
at the columns the prompts need ("trimmed", ``--tokens`` real tokens in the longest prompt, the others shorter) and at 77 padded columns
(``pad_to_max_length``, what upstream's tokenizer call produces), eager (``embed_tokens``: host validation, two small copies, the engine) and
the engine alone replayed from a captured graph (``embed_device``).  With the launch count and the effective weight bandwidth: at these row
counts the encoder is one pass over its weights (12 layers of 7.1 M floats, the pooler and the projection: about 343 MB) per call.

Device events around `--steps` calls after `--warmup` calls, `--rounds` alternating rounds, the median per leg.  No speed is gated anywhere:
this is where the number gets written down (profiles/clap_text_bench.txt).

    python tools/clap_text_bench.py [--prompts 1 8 16] [--tokens 16] [--steps 10] [--warmup 3] [--rounds 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from dataclasses import replace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import clap_ref  # noqa: E402
from syncfusion_amd.clap_text import ClapEmbedder, ClapTextConfig  # noqa: E402


def time_loop(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        step()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def engine_launches(cfg: ClapTextConfig) -> int:
    """Kernel launches of sf_clap_text_forward: the embedding gather, 7 per layer (qkv, attention, output + residual, LayerNorm, intermediate +
    GELU, output + residual, LayerNorm), 4 for the tail (pooler, two Linears, normalisation)."""
    return 1 + 7 * cfg.layers + 4


def streamed_weight_bytes(cfg: ClapTextConfig) -> int:
    """The weights one call reads whatever the batch: every layer, the pooler and the projection (the embedding tables are gathered by row)."""
    C, I, J = cfg.hidden, cfg.intermediate, cfg.joint_dim
    per_layer = 4 * C * C + 4 * C + 2 * C * I + I + C + 4 * C
    return 4 * (cfg.layers * per_layer + C * C + C + J * C + J + J * J + J)


def prompts(cfg: ClapTextConfig, B: int, longest: int, columns: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((B, columns), cfg.pad_id, dtype=torch.int64)
    mask = torch.zeros((B, columns), dtype=torch.int64)
    for b in range(B):
        n = longest if b == 0 else max(2, longest - (3 * b) % max(1, longest - 2))
        ids[b, 0], ids[b, n - 1] = cfg.bos_id, cfg.eos_id
        ids[b, 1:n - 1] = torch.randint(4, cfg.vocab_size, (n - 2,), generator=g)
        mask[b, :n] = 1
    return ids, mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompts", type=int, nargs="+", default=[1, 8, 16])
    ap.add_argument("--tokens", type=int, default=16, help="real tokens of the longest prompt, <s> and </s> included")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = ClapTextConfig()
    models = {"trimmed": ClapEmbedder(clap_ref.NARROW, cfg).to(dev), "padded_77": ClapEmbedder(clap_ref.NARROW, replace(cfg, pad_to_max_length=True)).to(dev)}
    weight_mb = streamed_weight_bytes(cfg) / 1e6
    text_params = sum(p.numel() for k, p in models["trimmed"].named_parameters() if ".text_" in k)
    out = {"engine_launches_per_call": engine_launches(cfg), "streamed_weight_MB": round(weight_mb, 1), "text_params_M": round(text_params / 1e6, 2),
           "longest_prompt_tokens": a.tokens}
    print(f"engine launches per call: {out['engine_launches_per_call']}; weights streamed per call: {weight_mb:.1f} MB; text parameters {out['text_params_M']} M",
          flush=True)
    with torch.no_grad():
        for B in a.prompts:
            ids, mask = prompts(cfg, B, a.tokens, cfg.max_length, 3 + B)
            legs, keep = {}, []
            for name, model in models.items():
                S = a.tokens if name == "trimmed" else cfg.max_length
                dids, dmask = ids[:, :S].to(torch.int32).contiguous().to(dev), mask[:, :S].to(torch.int32).contiguous().to(dev)
                eager = lambda model=model: model.embed_tokens(ids, mask)                            # noqa: E731
                device_part = lambda model=model, dids=dids, dmask=dmask: model.embed_device(dids, dmask)   # noqa: E731
                assert torch.equal(eager(), device_part())
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    device_part()
                torch.cuda.current_stream().wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    captured = device_part()
                graph.replay()
                assert torch.equal(captured, eager())
                keep.append((graph, captured, dids, dmask))
                legs[f"{name}_eager"] = eager
                legs[f"{name}_graph_replay"] = graph.replay
            same = float((models["trimmed"].embed_tokens(ids, mask) - models["padded_77"].embed_tokens(ids, mask)).abs().max())
            runs = {k: [] for k in legs}
            for _ in range(max(1, a.rounds)):
                for name, step in legs.items():
                    runs[name].append(time_loop(step, a.steps, a.warmup))
            res = {"max_abs_trimmed_minus_padded": same}
            for name, ms_all in runs.items():
                med = sorted(ms_all)[len(ms_all) // 2]
                rows = B * (a.tokens if name.startswith("trimmed") else cfg.max_length)
                res[name] = {"ms": round(med, 3), "rows": rows, "weight_GBps": round(weight_mb / med, 1), "rounds_ms": [round(v, 3) for v in ms_all]}
                print(f"prompts {B:2d} {name:24s}: {med:8.3f} ms  rows {rows:5d}  effective weight stream {weight_mb / med:7.1f} GB/s  "
                      f"(rounds {', '.join(f'{v:.3f}' for v in ms_all)})", flush=True)
            out[f"B{B}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
