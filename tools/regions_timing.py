"""smoothness-constrained regions of the voxel graph on the NeighborIndex (GPU box only): config 2's scene at --points
points, e = 0.1 (about 10^6 voxels at the default), radii of 1.5 and 3 edges, voxel_weight = point_counts().  normals
and seeds by smooth_regions' recipe (multiscale.voxel_normals at the same radius, max_curvature MAX_CURVATURE), made
once per radius outside the timed calls; max_angle MAX_ANGLE.  per radius and repetition, alternating on one card, whole
calls:
  regions_r*     NeighborIndex.regions (the kernels, the allocations and the one host read of the counts)
  components_r*  NeighborIndex.components with the same weights on the same handle
  dbscan_r*      NeighborIndex.dbscan with the same weights and dbscan_timing.py's min_weight
and once per radius, from lists(voxels(), radius): how many seed-seed edges of the graph pass and fail the normal test.
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
MAX_ANGLE = 0.26            # 15 degrees
MAX_CURVATURE = 0.05


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def edge_counts(index, radius, normals, seed, min_cos, chunk=1 << 18):
    """(seed-seed edges, passing, failing) of the graph at `radius`, every edge once, from the lists - in chunks of
    query voxels, so that no list of the whole graph is held"""
    voxels = index.voxels()
    total = passing = 0
    for lo in range(0, voxels.shape[0], chunk):
        offsets, other = index.lists(voxels[lo:lo + chunk], radius)
        own = torch.repeat_interleave(torch.arange(lo, lo + offsets.numel() - 1, device=other.device),
                                      offsets[1:] - offsets[:-1])
        keep = (other > own) & seed[own] & seed[other]
        a, b = normals[own[keep]], normals[other[keep]]
        dot = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
        total += int(keep.sum())
        passing += int((dot.abs() >= min_cos).sum())
    return total, passing, total - passing


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_750_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-edges", action="store_true", help="skip the edge census")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.points
    pts, _, _, _ = synth.make_config("c2_scene_1m", n=n)
    edge = 0.1
    dev = torch.from_numpy(pts).cuda()
    index = multiscale.NeighborIndex(dev, edge, method="index")
    weight = index.point_counts()
    m = index.n_voxels
    min_cos = multiscale._min_cos(MAX_ANGLE)

    calls, inputs = {}, {}
    for rho in RADII_IN_EDGES:
        r = rho * edge
        normals, seed = multiscale.voxel_normals(index, r, MAX_CURVATURE)
        inputs[rho] = (normals, seed)
        calls["regions_r%g" % rho] = lambda r=r, normals=normals, seed=seed: index.regions(
            r, voxel_normal=normals, max_angle=MAX_ANGLE, voxel_seed=seed, voxel_weight=weight)
        calls["components_r%g" % rho] = lambda r=r: index.components(r, voxel_weight=weight)
        calls["dbscan_r%g" % rho] = lambda r=r, k=MIN_POINTS[rho]: index.dbscan(r, k, voxel_weight=weight)
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
                if key.startswith("regions"):
                    facts[key + "_seeds"] = int(out[2].sum())
                    facts[key + "_attached"] = int(((labels >= 0) & ~out[2]).sum())
                    facts[key + "_unlabelled"] = int((labels < 0).sum())
            del out

    result = {"tool": "regions_timing", "config": "c2_scene_1m", "points": n, "edge": edge, "voxels": m,
              "radii_in_edges": list(RADII_IN_EDGES), "max_angle": MAX_ANGLE, "max_curvature": MAX_CURVATURE,
              "min_points": {"%g" % k: v for k, v in MIN_POINTS.items()}, "reps": args.reps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0)}
    result.update(facts)
    for key, ts in times.items():
        ts = sorted(ts)
        result[key + "_ms"] = {"median": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3), "max": round(ts[-1], 3)}
    if not args.no_edges:
        for rho in RADII_IN_EDGES:
            normals, seed = inputs[rho]
            total, passing, failing = edge_counts(index, rho * edge, normals, seed, min_cos)
            result["edges_r%g" % rho] = {"seed_seed": total, "pass": passing, "fail": failing}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
