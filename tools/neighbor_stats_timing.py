"""neighborhood statistics on the NeighborIndex against the field operator (GPU box only): config 2's cloud, one
scale (e = 0.1, r = 0.3), 4 attribute columns, query = search.  per repetition, alternating on one card:
  field          fields.vector_field_mean_gpu for that scale (nm_field_mean: rebuilds everything per call)
  build_table    NeighborIndex + members + voxel_table (what a new search cloud costs, once)
  stats          neighborhood_stats alone (what every further radius or query cloud costs)
  lists_gather   lists() + a torch gather-and-mean of the same columns (what not writing the lists saves)
prints one JSON line with the median and the spread of each; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nimrud_amd import synth  # noqa: E402
from nimrud_amd.minimal import fields, multiscale  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--dims", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, dims = args.points, args.dims
    pts, _, edges, radii = synth.make_config("c2_scene_1m", n=n)
    edge, radius = 0.1, 0.3
    dev = torch.from_numpy(pts).cuda()
    attr = torch.rand((n, dims), dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(7))

    def build_table():
        index = multiscale.NeighborIndex(dev, edge)
        index.members()
        return index, index.voxel_table(attr)

    def lists_gather(index, table):
        offsets, idx = index.lists(dev, radius)
        counts = offsets[1:] - offsets[:-1]
        owner = torch.repeat_interleave(torch.arange(n, device=dev.device), counts)
        total = torch.zeros((n, dims), dtype=torch.float64, device=dev.device).index_add_(0, owner, table[idx])
        return total / counts.clamp(min=1).unsqueeze(1)

    times = {"field": [], "build_table": [], "stats": [], "lists_gather": []}
    for rep in range(args.warmup + args.reps):
        t_field, field = timed(lambda: fields.vector_field_mean_gpu(dev, dev, attr, [edge], [radius]))
        t_build, (index, table) = timed(build_table)
        t_stats, (count, mean, vmin, vmax) = timed(lambda: index.neighborhood_stats(dev, radius, table))
        t_lists, gathered = timed(lambda: lists_gather(index, table))
        if rep >= args.warmup:
            for key, t in zip(("field", "build_table", "stats", "lists_gather"), (t_field, t_build, t_stats, t_lists)):
                times[key].append(t)
    # the three paths compute the same means, up to how a sum is ordered and a voxel mean is rounded
    scale = max(1.0, float(field.abs().max()))
    result = {"tool": "neighbor_stats_timing", "config": "c2_scene_1m", "points": n, "dims": dims, "edge": edge,
              "radius": radius, "voxels": index.n_voxels, "neighbors": int(count.sum()), "reps": args.reps,
              "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
              "max_abs_diff_stats_vs_field": float((mean - field).abs().max()),
              "max_abs_diff_gather_vs_stats": float((gathered - mean).abs().max()), "value_scale": scale}
    for key, ts in times.items():
        ts = sorted(ts)
        result[key + "_ms"] = {"median": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3), "max": round(ts[-1], 3)}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
