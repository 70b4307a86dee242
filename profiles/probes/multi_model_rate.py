"""Several FC models over one image set: one multi-model call (MultiContext, fused_fc_multi_kernel) against the K single-model
calls (bnm_infer_device) on the same images, HIP events, the two forms alternated in one process.

  python profiles/probes/multi_model_rate.py [--images 100000000] [--reps 5] [--sets small,zoo] [--json out.json]

Sets: small = fc_4bitsym_64, mcu_12k, mcu_12k_fp130, mcu_1k; zoo = the ten FC models of the zoo.  The images are synthetic
(DIST_M), resident in HBM, warmed by one call of each form first.  Prints per set the median ms of each form, their ratio
(multi / sum of singles) and the multi object's passes over the images (groups).  For counters, run it under
`rocprofv3 --kernel-trace --stats` and, separately, `rocprofv3 --kernel-trace --pmc FETCH_SIZE` (--reps 1): the multi kernel's
FETCH_SIZE should be about 256 B x n x groups plus the weights.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import bitnetmcu_amd as b  # noqa: E402

SETS = {
    "small": ["fc_4bitsym_64", "mcu_12k", "mcu_12k_fp130", "mcu_1k"],
    "zoo": ["fc_4bitsym_64", "mcu_12k", "mcu_12k_fp130", "mcu_1k", "tern_96", "tern_96_sparse", "doc12k_binary", "doc12k_ternary",
            "doc12k_2bit", "doc12k_8bit"],
}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sets", default="small,zoo")
    ap.add_argument("--json")
    ap.add_argument("--detail", action="store_true", help="also time each model alone and each adjacent pair as a multi object")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    n = a.images
    imgs = torch.empty((n, 256), dtype=torch.int8, device="cuda:0")
    b.synth.fill_device(imgs, first=0, dist=b.DIST_M)
    out = {}
    for set_name in a.sets.split(","):
        names = SETS[set_name]
        models = [b.Model.from_zoo(m) for m in names]
        mc = b.MultiContext(models, device=0)
        singles = [b.Context(m, device=0) for m in models]
        cls = torch.empty((len(models), n), dtype=torch.int32, device="cuda:0")

        def multi():
            mc.infer_device(imgs, cls)

        def single():
            for r, ctx in enumerate(singles):
                ctx.infer_device(imgs, cls[r])

        multi(); single()      # warm: kernels loaded, counter blocks allocated
        torch.cuda.synchronize()
        tm, ts = [], []
        for _ in range(a.reps):
            tm.append(timed(multi))
            ts.append(timed(single))
        per_model = []
        if a.detail:      # each model's single call, and the multi object of each adjacent pair
            for r, ctx in enumerate(singles):
                per_model.append(statistics.median([timed(lambda: ctx.infer_device(imgs, cls[r])) for _ in range(3)]))
            for r in range(len(models) - 1):
                pm = b.MultiContext(models[r:r + 2], device=0)
                pm.infer_device(imgs, cls)
                t = statistics.median([timed(lambda: pm.infer_device(imgs, cls)) for _ in range(3)])
                print(f"  pair {names[r]} + {names[r + 1]}: groups={pm.groups} {t:.2f} ms (singles {per_model[r]:.2f} + "
                      f"{per_model[r + 1]:.2f})", flush=True)
                pm.close()
        res = {"models": names, "single_ms_each": per_model, "images": n, "groups": mc.groups, "multi_ms": statistics.median(tm), "singles_ms": statistics.median(ts),
               "multi_all": tm, "singles_all": ts}
        res["ratio"] = res["multi_ms"] / res["singles_ms"]
        res["multi_images_per_s"] = n / (res["multi_ms"] * 1e-3)
        print(f"{set_name}: k={len(names)} groups={mc.groups} multi {res['multi_ms']:.2f} ms  singles {res['singles_ms']:.2f} ms  "
              f"ratio {res['ratio']:.3f}", flush=True)
        out[set_name] = res
        mc.close()
        for c in singles:
            c.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
