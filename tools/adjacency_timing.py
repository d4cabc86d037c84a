"""the adjacency of a labelling and prominence-merged peaks on the NeighborIndex (GPU box only): config 2's scene at
--points points, e = 0.1 (about 10^6 voxels at the default), radii of 1, 2 and 3 edges.  the value of a voxel is the
maximum z of its points (voxel_table, made once outside the timed calls), the labelling hill_climb's on that value.
per radius and repetition, alternating on one card in one process:
  hill_climb_r*       NeighborIndex.hill_climb(link="highest"), whole call - the nearest relative: one full-window walk
  adjacency_r*        NeighborIndex.adjacency(labels, value), whole call (two walks of the forward half-window, the sort
                      of the records' keys, the reduction; two host reads)
  peaks_r*            NeighborIndex.prominent_peaks(min_prominence = --prominence), whole call
  stage_*_r*          the same two calls once more with a synchronisation behind every stage: count (the first walk and
                      its scan, up to the host's read of the record count), emit (the second walk), sort (torch.sort of
                      the keys), reduce (heads, scan, segmented reduction, the read of the row count); for peaks also
                      hill_climb, merge (the copy down, nm_merge_by_prominence on the host) and relabel (the copy up
                      and the integer torch indexing).  the stages add up to more than the whole call: they wait.
and once per radius the number of segments, rows and crossing edges, and of segments after the merge.
prints one JSON line with the median and the spread of each; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nimrud_amd import _ffi, synth  # noqa: E402
from nimrud_amd.minimal import multiscale  # noqa: E402

RADII_IN_EDGES = (1.0, 2.0, 3.0)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


class Stages(object):
    """the callable the device methods report the end of a stage to: waits for the card and takes the time"""

    def __init__(self):
        self.ms = {}
        torch.cuda.synchronize()
        self.t0 = time.perf_counter()

    def __call__(self, name):
        torch.cuda.synchronize()
        now = time.perf_counter()
        self.ms[name] = self.ms.get(name, 0.0) + (now - self.t0) * 1e3
        self.t0 = now


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_750_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--prominence", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.points
    pts, _, _, _ = synth.make_config("c2_scene_1m", n=n)
    edge = 0.1
    dev = torch.from_numpy(pts).cuda()
    index = multiscale.NeighborIndex(dev, edge, method="index")
    m = index.n_voxels
    top = index.voxel_table(dev[:, 2], reduce="max")[:, 0].contiguous()
    mode = _ffi.NM_CLIMB["highest"]

    times, facts = {}, {}
    for rho in RADII_IN_EDGES:
        r = rho * edge
        tag = "_r%g" % rho
        labels = index.hill_climb(r, top, "highest")[0]
        pair, links, saddle = index.adjacency(r, labels, top)
        facts["segments" + tag] = int(labels.max()) + 1
        facts["rows" + tag] = int(pair.shape[0])
        facts["crossing_edges" + tag] = int(links.sum())
        facts["segments_after_merge" + tag] = int(index.prominent_peaks(r, top, args.prominence)[1].shape[0])
        del pair, links, saddle

        def staged_adjacency(r=r, labels=labels):
            stages = Stages()
            index._adjacency_device(r, labels, top, None, stages)
            return stages.ms

        def staged_peaks(r=r):
            stages = Stages()
            index._prominent_peaks_device(r, top, mode, args.prominence, None, None, 1, stages)
            return stages.ms

        calls = {
            "hill_climb" + tag: lambda r=r: index.hill_climb(r, top, "highest"),
            "adjacency" + tag: lambda r=r, labels=labels: index.adjacency(r, labels, top),
            "peaks" + tag: lambda r=r: index.prominent_peaks(r, top, args.prominence),
        }
        for rep in range(args.warmup + args.reps):
            for key, fn in calls.items():
                t, out = timed(fn)
                del out
                if rep >= args.warmup:
                    times.setdefault(key, []).append(t)
            for what, fn in (("adjacency", staged_adjacency), ("peaks", staged_peaks)):
                for name, t in fn().items():
                    if rep >= args.warmup:
                        times.setdefault("stage_%s_%s%s" % (what, name, tag), []).append(t)
        del labels

    result = {"tool": "adjacency_timing", "config": "c2_scene_1m", "points": n, "edge": edge, "voxels": m,
              "radii_in_edges": list(RADII_IN_EDGES), "value": "max z per voxel", "labels": "hill_climb, highest",
              "min_prominence": args.prominence, "reps": args.reps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0)}
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
