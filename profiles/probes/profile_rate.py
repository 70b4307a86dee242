#!/usr/bin/env python3
"""Images/s of a profiled call (bnm_infer_device_profiled) against a plain one (bnm_infer_device) on resident int8 images.

  python profiles/probes/profile_rate.py --model fc_4bitsym_64 --n 100000000
  python profiles/probes/profile_rate.py --model cnn_64 --n 10000000

One process per model; it writes one JSON line to stdout and to --out.  Each form is warmed up once, then timed --reps times with
device events around the call (the median is reported).
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="fc_4bitsym_64")
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import bitnetmcu_amd as b
    model = b.Model.from_zoo(a.model)
    ctx = b.Context(model, device=0)
    n = a.n
    x = torch.empty((n, 256), dtype=torch.int8, device="cuda:0")
    b.synth.fill_device(x, first=0, dist=b.DIST_U)
    cls = torch.empty(n, dtype=torch.int32, device="cuda:0")
    ctr = torch.zeros(ctx.profile_words(), dtype=torch.int64, device="cuda:0")

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 1e3)
        return sorted(ts)[len(ts) // 2]

    res = {"model": a.model, "n": n}
    t = timed(lambda: ctx.infer_device(x, cls))
    res["plain_s"], res["plain_img_s"], res["plain_kernels"] = t, n / t, ctx.last_kernel
    for mode in (0, 2):
        ctx.set_profile_mode(mode)
        t = timed(lambda: ctx.profile_device(x, ctr, cls=cls))
        res[f"mode{mode}_s"], res[f"mode{mode}_img_s"], res[f"mode{mode}_kernels"] = t, n / t, ctx.last_kernel
    try:
        ctx.set_profile_mode(1)
        res["mode1"] = "accepted"
    except b.BnmError as e:
        res["mode1"] = f"refused: {e}"
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
