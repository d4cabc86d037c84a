"""k nearest voxels on the NeighborIndex (GPU box only): config 2's cloud, e = 0.1, query = search.  per repetition,
alternating on one card, whole calls:
  nearest_k{1,8,32}        NeighborIndex.nearest without a limit (squared=True: the kernels and the allocations)
  nearest_k{1,8,32}_r0.3   the same with max_distance = 0.3 (the near stage alone: the limit's window is 3 cells)
  lists_r0.3               the handle's own lists() at r = 0.3 (two walks and a cumsum)
and once, on the host with 16 workers, scipy.spatial.cKDTree.query on the first --tree-rows rows (the tree is built
outside the timing).  `pending_k*` is how many queries the near stage handed to the wide stage.
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

KS = (1, 8, 32)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tree-rows", type=int, default=100_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.points
    pts, _, _, _ = synth.make_config("c2_scene_1m", n=n)
    edge, radius = 0.1, 0.3
    dev = torch.from_numpy(pts).cuda()
    _, index = timed(lambda: multiscale.NeighborIndex(dev, edge))
    rt = index._rt

    calls = {}
    for k in KS:
        calls["nearest_k%d" % k] = lambda k=k: index.nearest(dev, k, squared=True)
        calls["nearest_k%d_r%g" % (k, radius)] = lambda k=k: index.nearest(dev, k, max_distance=radius, squared=True)
    calls["lists_r%g" % radius] = lambda: index.lists(dev, radius)
    times = {key: [] for key in calls}
    pending, found = {}, {}
    for rep in range(args.warmup + args.reps):
        for key, fn in calls.items():
            t, out = timed(fn)
            if rep >= args.warmup:
                times[key].append(t)
            if rep == 0 and key.startswith("nearest") and "_r" not in key:
                # the scratch still holds what the near stage listed for the wide stage
                word = rt.workspace(4)[:4].cpu().numpy().view(np.uint32)
                pending["pending_" + key[8:]] = int(word[0])
            if rep == 0 and key.startswith("nearest"):
                found["mean_found_" + key[8:]] = round(float((out[1] >= 0).sum()) / n, 3)

    result = {"tool": "nearest_timing", "config": "c2_scene_1m", "points": n, "edge": edge, "max_distance": radius,
              "voxels": index.n_voxels, "reps": args.reps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0)}
    result.update(pending)
    result.update(found)
    for key, ts in times.items():
        ts = sorted(ts)
        result[key + "_ms"] = {"median": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3), "max": round(ts[-1], 3)}

    # the host's answer to the same question, on a slice
    from scipy.spatial import cKDTree
    voxels = index.voxels().cpu().numpy()
    rows = pts[:args.tree_rows, :3]
    tree = cKDTree(voxels, leafsize=300)
    result["ckdtree"] = {"rows": len(rows), "workers": 16, "leafsize": 300}
    for k in KS:
        for limit in (np.inf, radius):
            t0 = time.perf_counter()
            dist, idx = tree.query(rows, k, distance_upper_bound=limit, workers=16)
            ms = (time.perf_counter() - t0) * 1e3
            result["ckdtree"]["k%d%s_ms" % (k, "" if np.isinf(limit) else "_r%g" % limit)] = round(ms, 3)
    # same voxels, wherever nothing ties (the order of exact ties is scipy's own)
    got = index.nearest(dev[:args.tree_rows], 1, squared=True)[1].cpu().numpy()[:, 0]
    result["ckdtree"]["k1_index_mismatches"] = int((tree.query(rows, 1, workers=16)[1] != got).sum())
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
