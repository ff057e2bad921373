"""Cross-attention from the voxels of a sparse tensor to a dense context (csrc/attention.hip, ABI 1.20): time per call of
MinkowskiCrossAttentionFunction, forward and forward + backward with all three gradients, with the dK / dV pass at the
policy's number of query slices S (me_attn_kv_splits), at a forced S = 1 (the key-stationary kernel alone: the yardstick
of the split) and at two other forced values, next to the torch formulation a user writes without it.

    python scripts/cross_attention_bench.py [--iters 50] [--repeats 3] [--json out.jsonl]

Protocol of scripts/attention_bench.py: 10 warm-up calls, then `iters` calls between two device events; every figure is
taken `repeats` times, the variants alternating inside a repeat, and printed as min-max.
  ours    MinkowskiCrossAttentionFunction on q [N, C] and k, v [B, L, C] with context_lengths (the query lists are cached in
          the manager; the context lists are built per call, one launch)
  padded  the queries of every instance padded to the longest one, one scaled_dot_product_attention with a key mask from
          the lengths; the index lists are built outside the timed region
Shapes: 2 x 20,000 voxels and 8 unequal scenes summing to 20,000; C = 256 with 8 and 4 heads; L = 77 (CLIP text) and
1,374 (DINO patches); every second context is padded by a quarter.  Dtypes: bf16 and fp32."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import _lib
from attention_bench import make_coords, timed

SCENES = (("2x20000", [20000, 20000]), ("8 unequal", [5200, 4100, 3300, 2600, 2000, 1400, 900, 500]))
FORCED = (1, 4, 16)


def case(name, sizes, C, heads, tokens, dtype, iters, repeats, dev):
    x = ME.SparseTensor(torch.zeros(sum(sizes), 1), coordinates=make_coords(sizes, True), device=dev)
    batch = x.C[:, 0].long()
    n, B, d = batch.numel(), len(sizes), C // heads
    q = torch.randn(n, C, device=dev).to(dtype).requires_grad_(True)
    k, v = (torch.randn(B, tokens, C, device=dev).to(dtype).requires_grad_(True) for _ in range(2))
    dout = torch.randn(n, C, device=dev).to(dtype)
    lengths = torch.tensor([tokens if b % 2 == 0 else (3 * tokens) // 4 for b in range(B)], device=dev)
    key, mgr = x.coordinate_map_key, x.coordinate_manager
    rows = [(batch == b).nonzero().reshape(-1) for b in range(B)]                 # outside the timed region
    longest = max(sizes)
    pad_index = torch.zeros(B, longest, dtype=torch.long, device=dev)
    pad_valid = torch.zeros(B, longest, dtype=torch.bool, device=dev)
    for b, r in enumerate(rows):
        pad_index[b, :r.numel()] = r
        pad_valid[b, :r.numel()] = True
    flat_valid = pad_valid.reshape(-1).nonzero().reshape(-1)
    key_mask = (torch.arange(tokens, device=dev)[None] < lengths[:, None])[:, None, None, :]
    sdpa = torch.nn.functional.scaled_dot_product_attention

    def ours(splits=None):
        return lambda: ME.MinkowskiCrossAttentionFunction.apply(q, k, v, lengths, heads, None, key, mgr, splits)

    def padded():
        qb = q[pad_index.reshape(-1)].view(B, longest, heads, d).transpose(1, 2)
        kb, vb = (t.view(B, tokens, heads, d).transpose(1, 2) for t in (k, v))
        o = sdpa(qb, kb, vb, attn_mask=key_mask).transpose(1, 2).reshape(-1, C)
        return torch.empty_like(q).index_copy(0, pad_index.reshape(-1)[flat_valid], o[flat_valid])

    def step(fwd):
        def run():
            q.grad = k.grad = v.grad = None
            fwd().backward(dout)
        return run

    def spans(fns):
        """every function `repeats` times, the functions alternating inside a repeat -> {name: [min, max] us}"""
        t = {nm: [] for nm in fns}
        for _ in range(repeats):
            for nm, fn in fns.items():
                t[nm].append(timed(fn, iters) * 1e6)
        return {nm: [round(min(v), 1), round(max(v), 1)] for nm, v in t.items()}
    policy = int(_lib.load().me_attn_kv_splits(n, B * tokens, B, C, heads))
    step(ours())()
    res, dk = ours()().detach().float(), k.grad.float().clone()
    step(padded)()
    r = dict(scenes=name, C=C, heads=heads, tokens=tokens, dtype="bf16" if dtype == torch.bfloat16 else "f32", n=n,
             policy_S=policy, out_diff_padded=float((res - padded().detach().float()).abs().max()),
             dk_diff_padded=float((dk - k.grad.float()).abs().max()))
    with torch.no_grad():
        fwd = spans(dict(ours=ours(), padded=padded))
    steps = dict(policy=step(ours()), padded=step(padded))
    steps.update({str(s): step(ours(s)) for s in FORCED})
    steps = spans(steps)
    r.update(ours_fwd_us=fwd["ours"], padded_fwd_us=fwd["padded"], padded_step_us=steps.pop("padded"), ours_step_us=steps)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert args.iters >= 20 and args.repeats >= 1
    dev = torch.device("cuda:0")
    results = []
    for name, sizes in SCENES:
        for heads in (8, 4):
            for tokens in (77, 1374):
                for dt in (torch.bfloat16, torch.float32):
                    r = case(name, sizes, 256, heads, tokens, dt, args.iters, args.repeats, dev)
                    results.append(r)
                    print(json.dumps(r), flush=True)
    fmt = lambda p: f"{p[0]:8.1f}-{p[1]:<8.1f}"       # noqa: E731
    print(f"{'scenes':10s} {'H':>2s} {'L':>5s} {'dtype':5s} | fwd us {'ours':>17s} {'padded':>17s} | fwd+bwd us "
          f"{'S=policy':>17s} " + " ".join(f"{'S=' + str(s):>17s}" for s in FORCED) + f" {'padded':>17s} | policy S")
    for r in results:
        print(f"{r['scenes']:10s} {r['heads']:2d} {r['tokens']:5d} {r['dtype']:5s} |        {fmt(r['ours_fwd_us'])} "
              f"{fmt(r['padded_fwd_us'])} |            {fmt(r['ours_step_us']['policy'])} " +
              " ".join(fmt(r['ours_step_us'][str(s)]) for s in FORCED) + f" {fmt(r['padded_step_us'])} | {r['policy_S']}")
    if args.json:
        with open(args.json, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
