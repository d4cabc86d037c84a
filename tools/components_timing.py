"""connected components of the voxel graph on the NeighborIndex (GPU box only): config 2's scene at --points points,
e = 0.1 (about 10^6 voxels at the default), radii of 1.5 and 3 edges.  per radius and repetition, alternating on one
card, whole calls:
  components_r*          NeighborIndex.components (the kernels, the allocations and the one host read of the counts)
  components_weighted_r* the same with voxel_weight = point_counts() and min_size = 10
  lists_r*               the handle's own lists(voxels(), r): what the only route without components() starts with
and once per radius, that route to its end: the download of the lists and scipy.sparse.csgraph.connected_components
on one core (`route_*`: its three parts in ms).  the component count of both ways is compared.
prints one JSON line with the median and the spread of each; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nimrud_amd import synth  # noqa: E402
from nimrud_amd.minimal import multiscale  # noqa: E402

RADII_IN_EDGES = (1.5, 3.0)


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
    ap.add_argument("--no-scipy", action="store_true", help="skip the download + scipy leg")
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
        calls["components_r%g" % rho] = lambda r=r: index.components(r)
        calls["components_weighted_r%g" % rho] = lambda r=r: index.components(r, voxel_weight=weight, min_size=10)
        calls["lists_r%g" % rho] = lambda r=r: index.lists(voxels, r)
    times = {key: [] for key in calls}
    facts = {}
    for rep in range(args.warmup + args.reps):
        for key, fn in calls.items():
            t, out = timed(fn)
            if rep >= args.warmup:
                times[key].append(t)
            if rep == 0 and key.startswith("components"):
                facts[key + "_count"] = int(out[1].shape[0])
                facts[key + "_largest"] = int(out[1].max()) if out[1].numel() else 0
            if rep == 0 and key.startswith("lists"):
                facts[key + "_neighbors_per_voxel"] = round(float(out[1].shape[0]) / max(m, 1), 2)
            del out

    result = {"tool": "components_timing", "config": "c2_scene_1m", "points": n, "edge": edge, "voxels": m,
              "radii_in_edges": list(RADII_IN_EDGES), "reps": args.reps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0)}
    result.update(facts)
    for key, ts in times.items():
        ts = sorted(ts)
        result[key + "_ms"] = {"median": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3), "max": round(ts[-1], 3)}

    if not args.no_scipy:
        # the route of a handle without components(): the whole edge list, down to the host, scipy on one core
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import connected_components
        for rho in RADII_IN_EDGES:
            t_lists, (offsets, idx) = timed(lambda: index.lists(voxels, rho * edge))
            t0 = time.perf_counter()
            offsets_h, idx_h = offsets.cpu().numpy(), idx.cpu().numpy()
            t_down = (time.perf_counter() - t0) * 1e3
            del offsets, idx
            t0 = time.perf_counter()
            graph = csr_matrix((np.ones(len(idx_h), dtype=np.int8), idx_h, offsets_h), shape=(m, m))
            count, _ = connected_components(graph, directed=False)
            t_scipy = (time.perf_counter() - t0) * 1e3
            result["route_r%g" % rho] = {"lists_ms": round(t_lists, 3), "download_ms": round(t_down, 3),
                                         "scipy_ms": round(t_scipy, 3), "edge_list_bytes": int(idx_h.nbytes),
                                         "components": int(count),
                                         "same_count": int(count) == facts["components_r%g_count" % rho]}
            del graph, offsets_h, idx_h
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
