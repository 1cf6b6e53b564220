"""Micro-benchmark of the limited-context attention kernels (csrc/attn_fused.hip / attn_bwd.hip CTX) against the
full-context register-staged kernels at the same shape: the single-pass forward (O + lse) and the whole bwd2
backward (dQ + dS / Pd, dK / dV, dPpos + fold).  Default: B=4, H=8, d=512, T=2001 (FastConformer on ~160 s of
audio), regular (128, 128), no dropout.  Warm-up, then `reps` back-to-back launches between two device events,
repeated `rounds` times (median and spread printed).
usage: python tools/attn_ctx_micro.py [reps] [rounds] [left right [chunked]]"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kd-via-fm-in-asr_amd"))
import torch  # noqa: E402

from kdfm import kernels as K  # noqa: E402
from kdfm.config import att_context_triple  # noqa: E402


def timed(fn, reps, rounds):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / reps * 1e3)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def main():
    a = sys.argv[1:]
    reps = int(a[0]) if len(a) > 0 else 50
    rounds = int(a[1]) if len(a) > 1 else 5
    size = (int(a[2]), int(a[3])) if len(a) > 3 else (128, 128)
    style = "chunked_limited" if len(a) > 4 else "regular"
    ctx = att_context_triple(size, style)
    B, H, T, d, p = 4, 8, 2001, 512, 0.0
    dk = d // H
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    rows = B * T
    qkv = torch.randn(rows, 3 * d, device=dev, generator=g)
    qu = torch.randn(rows, d, device=dev, generator=g)
    qv = torch.randn(rows, d, device=dev, generator=g)
    ppos = torch.randn(2 * T - 1, d, device=dev, generator=g)
    do = torch.randn(rows, d, device=dev, generator=g)
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)
    sc = 1.0 / math.sqrt(dk)
    o = torch.empty(rows, d, device=dev)
    lse = torch.empty(B, H, T, device=dev)
    o_c = torch.empty(rows, d, device=dev)
    lse_c = torch.empty(B, H, T, device=dev)
    dqu = torch.empty(rows, d, device=dev)
    dqv = torch.empty_like(dqu)
    dqkv = torch.zeros(rows, 3 * d, device=dev)
    dpos = torch.empty(2 * T - 1, d, device=dev)
    ds, pd = K.attn_bwd2_saved(B, H, T, dev)
    ws = torch.empty(K.relpos_attn_bwd2_dpos_ws(B, T, d), device=dev)

    def fwd_full():
        K.relpos_attn_fwd(qu, qv, qkv, ppos, lens, o, None, None, B, H, T, sc, p, None, 11, lse=lse)

    def fwd_ctx():
        K.relpos_attn_ctx_fwd(qu, qv, qkv, ppos, lens, o_c, B, H, T, sc, p, None, 11, ctx, lse=lse_c)

    def bwd_full():
        K.relpos_attn_bwd2_dq(do, o, qu, qv, qkv, ppos, lse, lens, None, ds, pd, dqu, dqv, B, H, T, sc, p, None, 11)
        K.relpos_attn_bwd2_dkv(do, qu, ds, pd, lens, dqkv, B, H, T)
        K.relpos_attn_bwd2_dpos(qv, ds, lens, dpos, B, H, T, ws=ws)

    def bwd_ctx():
        K.relpos_attn_ctx_bwd(do, o_c, qu, qv, qkv, ppos, lse_c, lens, dqu, dqv, dqkv, dpos, B, H, T, sc, p, None, 11,
                              ctx, ds=ds, pd=pd, ws=ws)

    nb = (T + 63) // 64
    print(f"B={B} H={H} T={T} d={d} ctx={size} {style}: {K.ctx_tiles(T, ctx)} of {nb * nb} tiles per (b, h)", flush=True)
    res = {}
    for name, fn in (("fwd full", fwd_full), ("fwd ctx", fwd_ctx), ("bwd full", bwd_full), ("bwd ctx", bwd_ctx)):
        res[name] = timed(fn, reps, rounds)
        med, lo, hi = res[name]
        print(f"{name:10s} median {med:9.1f} us  (min {lo:9.1f}, max {hi:9.1f}; {rounds} x {reps} launches)", flush=True)
    print(f"forward  full / ctx = {res['fwd full'][0] / res['fwd ctx'][0]:.2f}x")
    print(f"backward full / ctx = {res['bwd full'][0] / res['bwd ctx'][0]:.2f}x")


if __name__ == "__main__":
    main()
