"""peak-seeking segments of the voxel graph on the NeighborIndex (GPU box only): config 2's scene at --points points,
e = 0.1 (about 10^6 voxels at the default), radii of 1.5 and 3 edges, voxel_weight = point_counts().  the value of a
voxel is the maximum z of its points (voxel_table, made once outside the timed calls).  per radius and repetition,
alternating on one card, whole calls:
  highest_r*     NeighborIndex.hill_climb(link="highest") (the kernels, the allocations, the one host read of the counts)
  nearest_r*     NeighborIndex.hill_climb(link="nearest")
  deep_r*        NeighborIndex.hill_climb(link="nearest") with the voxel's x as its value: every voxel steps about one
                 cell, so the chains k_cc_flatten follows run along the whole scene
  components_r*  NeighborIndex.components with the same weights on the same handle
and once per hill_climb call the number of segments, the largest one and the longest chain of links.
prints one JSON line with the median and the spread of each; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nimrud_amd import synth  # noqa: E402
from nimrud_amd.minimal import multiscale  # noqa: E402

RADII_IN_EDGES = (1.5, 3.0)
# the order of the calls of one repetition (tools/hill_climb_trace_summary.py splits the kernel trace by it)
ORDER = ("highest", "nearest", "deep", "components")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def longest_chain(link):
    """the largest number of links between a voxel and its peak, by pointer doubling"""
    at = torch.arange(link.shape[0], device=link.device)
    jump = torch.where(link >= 0, link, at)
    depth = (jump != at).to(torch.int64)
    while True:
        far = jump[jump]
        if torch.equal(far, jump):
            return int(depth.max()) if depth.numel() else 0
        depth = depth + depth[jump]
        jump = far


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_750_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.points
    pts, _, _, _ = synth.make_config("c2_scene_1m", n=n)
    edge = 0.1
    dev = torch.from_numpy(pts).cuda()
    index = multiscale.NeighborIndex(dev, edge, method="index")
    weight = index.point_counts()
    m = index.n_voxels
    top = index.voxel_table(dev[:, 2], reduce="max")[:, 0].contiguous()
    along = index.voxels()[:, 0].contiguous()

    calls = {}
    for rho in RADII_IN_EDGES:
        r = rho * edge
        calls["highest_r%g" % rho] = lambda r=r: index.hill_climb(r, top, "highest", voxel_weight=weight,
                                                                  return_link=True)
        calls["nearest_r%g" % rho] = lambda r=r: index.hill_climb(r, top, "nearest", voxel_weight=weight,
                                                                  return_link=True)
        calls["deep_r%g" % rho] = lambda r=r: index.hill_climb(r, along, "nearest", voxel_weight=weight,
                                                               return_link=True)
        calls["components_r%g" % rho] = lambda r=r: index.components(r, voxel_weight=weight)
    assert [key.split("_")[0] for key in calls] == list(ORDER) * len(RADII_IN_EDGES)
    times = {key: [] for key in calls}
    facts = {}
    for rep in range(args.warmup + args.reps):
        for key, fn in calls.items():
            t, out = timed(fn)
            if rep >= args.warmup:
                times[key].append(t)
            if rep == 0:
                sizes = out[1]
                facts[key + "_count"] = int(sizes.shape[0])
                facts[key + "_largest"] = int(sizes.max()) if sizes.numel() else 0
                facts[key + "_largest_share_of_points"] = round(facts[key + "_largest"] / float(n), 4)
                if not key.startswith("components"):
                    facts[key + "_longest_chain"] = longest_chain(out[3])
            del out

    result = {"tool": "hill_climb_timing", "config": "c2_scene_1m", "points": n, "edge": edge, "voxels": m,
              "radii_in_edges": list(RADII_IN_EDGES), "value": "max z per voxel (deep_*: the voxel's x)",
              "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    result.update(facts)
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
