"""the segment table (multiscale.segment_table) on config 2's scene at --points points (GPU box only), three labellings
of the same cloud, whole calls alternating on one card:
  giant   cluster_cloud's labels at e = 0.1, clustered at 1.5 edges: one segment holds most of the cloud
  even    row % 4096: 4096 segments of equal length, every one scattered over the whole cloud
  tiny    row // 3: a third of a million segments of three rows
and beside each the only route without the kernel: download cloud and labels, group the rows by label (a stable
argsort) and reduce every segment with numpy as tests/segments_reference.py does, on --workers processes that share
the segments out (`route_*`: its parts in ms; one segment is one process's work, however long it is).
prints one JSON line with the median and the spread of each; --out also writes it to a file."""
import argparse
import json
import multiprocessing
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402

_shared = {}


def _worker_init(path):
    data = np.load(path, mmap_mode="r")
    _shared["points"] = data


def _worker_reduce(job):
    import segments_reference as ref
    rows_path, lo, hi, starts = job
    rows = np.load(rows_path, mmap_mode="r")
    points = _shared["points"]
    out = np.zeros((hi - lo, ref.COLUMNS))
    for k in range(hi - lo):
        mine = rows[starts[k]:starts[k + 1]]
        if len(mine):
            out[k] = ref.segment_row(points[np.asarray(mine)])
    return lo, out


def cpu_route(pool, tmpdir, points_path, labels_h, c, workers):
    """(group_ms, reduce_ms, table): stable argsort by label, then the segments dealt out in `4 * workers` runs"""
    t0 = time.perf_counter()
    valid = np.nonzero((labels_h >= 0) & (labels_h < c))[0]
    rows = valid[np.argsort(labels_h[valid], kind="stable")]
    start = np.searchsorted(labels_h[rows], np.arange(c + 1))
    t_group = (time.perf_counter() - t0) * 1e3
    rows_path = os.path.join(tmpdir, "rows.npy")
    np.save(rows_path, rows)
    t0 = time.perf_counter()
    cuts = np.linspace(0, c, min(c, 4 * workers) + 1).astype(np.int64)
    jobs = [(rows_path, int(a), int(b), start[a:b + 1]) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    table = np.zeros((c, 25))
    for lo, part in pool.imap_unordered(_worker_reduce, jobs):
        table[lo:lo + len(part)] = part
    t_reduce = (time.perf_counter() - t0) * 1e3
    return t_group, t_reduce, table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_750_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--no-cpu", action="store_true", help="skip the download + numpy leg")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from nimrud_amd import synth
    from nimrud_amd.minimal import multiscale

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    n = args.points
    pts, _, _, _ = synth.make_config("c2_scene_1m", n=n)
    edge = 0.1
    dev = torch.from_numpy(pts).cuda()
    cluster_labels, sizes = multiscale.cluster_cloud(dev, edge, 1.5 * edge)
    row = torch.arange(n, device=dev.device)
    cases = {"giant": (cluster_labels, int(sizes.shape[0])), "even": (row % 4096, 4096),
             "tiny": (row // 3, (n + 2) // 3)}
    result = {"tool": "segments_timing", "config": "c2_scene_1m", "points": n, "edge": edge,
              "cluster_radius_in_edges": 1.5, "reps": args.reps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "chunk": 256,
              "giant_segments": int(sizes.shape[0]), "giant_largest": int(sizes.max()) if sizes.numel() else 0,
              "giant_unlabelled": int((cluster_labels < 0).sum())}
    times = {key: [] for key in cases}
    tables = {}
    for rep in range(args.warmup + args.reps):
        for key, (labels, c) in cases.items():
            t, out = timed(lambda: multiscale.segment_table(dev, labels, n_segments=c))
            if rep >= args.warmup:
                times[key].append(t)
            if rep == 0:
                tables[key] = out.cpu().numpy()
            elif rep == 1:
                result[key + "_repeats_bit_for_bit"] = bool(np.array_equal(out.cpu().numpy().view(np.uint64),
                                                                           tables[key].view(np.uint64)))
            del out
    for key, ts in times.items():
        ts = sorted(ts)
        result[key + "_ms"] = {"median": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3), "max": round(ts[-1], 3)}
        result[key + "_segments"] = cases[key][1]

    if not args.no_cpu:
        with tempfile.TemporaryDirectory() as tmpdir:
            points_path = os.path.join(tmpdir, "points.npy")
            np.save(points_path, pts[:, :3])
            ctx = multiprocessing.get_context("spawn")       # fresh processes: none of them inherits the GPU
            with ctx.Pool(args.workers, initializer=_worker_init, initargs=(points_path,)) as pool:
                pool.map(abs, range(args.workers))           # the workers are up before anything is timed
                for key, (labels, c) in cases.items():
                    t0 = time.perf_counter()
                    _, labels_h = dev.cpu().numpy(), labels.cpu().numpy()
                    t_down = (time.perf_counter() - t0) * 1e3
                    t_group, t_reduce, table = cpu_route(pool, tmpdir, points_path, labels_h, c, args.workers)
                    got = tables[key]
                    scale = np.abs(table).max(0) + 1e-300
                    result["route_" + key] = {
                        "download_ms": round(t_down, 3), "group_ms": round(t_group, 3), "reduce_ms": round(t_reduce, 3),
                        "workers": args.workers,
                        "n_and_box_equal": bool(np.array_equal(got[:, [0, 4, 5, 6, 7, 8, 9]],
                                                               table[:, [0, 4, 5, 6, 7, 8, 9]])),
                        "covariance_max_diff_over_column_max": float((np.abs(got[:, 10:16] - table[:, 10:16])
                                                                      / scale[10:16]).max())}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
