"""density-based clusters of the voxel graph on the NeighborIndex (GPU box only): config 2's scene at --points points,
e = 0.1 (about 10^6 voxels at the default), radii of 1.5 and 3 edges, voxel_weight = point_counts() and min_weight =
MIN_POINTS[radius] points.  per radius and repetition, alternating on one card, whole calls:
  dbscan_r*      NeighborIndex.dbscan (the kernels, the allocations and the one host read of the counts)
  components_r*  NeighborIndex.components with the same weights on the same handle: single linkage, what the handle
                 had before
and once per radius, on the CPU: sklearn.cluster.DBSCAN with sample_weight and --workers workers on the first
--slice voxels (`sklearn_r*`: ms, clusters, core voxels; the same slice through the numbers of dbscan() would be another
graph - voxels of the slice lose their neighbors outside it - so only the time is compared).
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
MIN_POINTS = {1.5: 12, 3.0: 40}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_750_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slice", type=int, default=100_000, help="voxels handed to sklearn")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--no-sklearn", action="store_true", help="skip the CPU leg")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.points
    pts, _, _, _ = synth.make_config("c2_scene_1m", n=n)
    edge = 0.1
    dev = torch.from_numpy(pts).cuda()
    index = multiscale.NeighborIndex(dev, edge, method="index")
    voxels = index.voxels()
    weight = index.point_counts()
    m = index.n_voxels

    calls = {}
    for rho in RADII_IN_EDGES:
        r = rho * edge
        calls["dbscan_r%g" % rho] = lambda r=r, k=MIN_POINTS[rho]: index.dbscan(r, k, voxel_weight=weight)
        calls["components_r%g" % rho] = lambda r=r: index.components(r, voxel_weight=weight)
    times = {key: [] for key in calls}
    facts = {}
    for rep in range(args.warmup + args.reps):
        for key, fn in calls.items():
            t, out = timed(fn)
            if rep >= args.warmup:
                times[key].append(t)
            if rep == 0:
                labels, sizes = out[0], out[1]
                facts[key + "_count"] = int(sizes.shape[0])
                facts[key + "_largest"] = int(sizes.max()) if sizes.numel() else 0
                facts[key + "_largest_share_of_points"] = round(facts[key + "_largest"] / float(n), 4)
                if key.startswith("dbscan"):
                    core = out[2]
                    facts[key + "_core"] = int(core.sum())
                    facts[key + "_border"] = int(((labels >= 0) & ~core).sum())
                    facts[key + "_noise"] = int((labels < 0).sum())
            del out

    result = {"tool": "dbscan_timing", "config": "c2_scene_1m", "points": n, "edge": edge, "voxels": m,
              "radii_in_edges": list(RADII_IN_EDGES), "min_points": {"%g" % k: v for k, v in MIN_POINTS.items()},
              "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    result.update(facts)
    for key, ts in times.items():
        ts = sorted(ts)
        result[key + "_ms"] = {"median": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3), "max": round(ts[-1], 3)}

    if not args.no_sklearn:
        from sklearn.cluster import DBSCAN
        k = min(args.slice, m)
        host_voxels = voxels[:k].cpu().numpy()
        host_weight = weight[:k].cpu().numpy()
        for rho in RADII_IN_EDGES:
            t0 = time.perf_counter()
            sk = DBSCAN(eps=rho * edge, min_samples=MIN_POINTS[rho], n_jobs=args.workers).fit(
                host_voxels, sample_weight=host_weight)
            t = (time.perf_counter() - t0) * 1e3
            result["sklearn_r%g" % rho] = {"ms": round(t, 3), "voxels": int(k), "workers": args.workers,
                                           "clusters": int(sk.labels_.max()) + 1,
                                           "core": int(len(sk.core_sample_indices_))}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
