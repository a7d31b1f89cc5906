"""Sweep a grid of noise parameters in one resident run: T tunings x W shared worlds = T W filters of one context
(xivo_amd/sweep.py, the tuning table of include/xivo_hip.h), and print one JSON line with the per-tuning table.

  python scripts/run_sweep.py -axis visual_meas_std=0.5:4:8 -axis MH_thresh=3,5.991,9 -worlds 16 -total_time 4
"""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_axis(text):
    """NAME=lo:hi:n (n values from lo to hi, linear) or NAME=v1,v2,... -> (NAME, [values])"""
    name, sep, spec = text.partition("=")
    name, spec = name.strip(), spec.strip()
    if not sep or not name or not spec:
        raise argparse.ArgumentTypeError("an axis is NAME=lo:hi:n or NAME=v1,v2,... (got %r)" % text)
    try:
        if ":" in spec:
            lo, hi, n = spec.split(":")
            n = int(n)
            if n < 1:
                raise ValueError
            return name, [float(v) for v in np.linspace(float(lo), float(hi), n)]
        return name, [float(v) for v in spec.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError("an axis is NAME=lo:hi:n or NAME=v1,v2,... (got %r)" % text)


def make_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-axis", action="append", type=parse_axis, default=[], metavar="NAME=lo:hi:n | NAME=v1,v2,...",
                    help="one axis of the grid (repeat for more; the last one varies fastest): a tunable field of SequenceConfig - "
                         "visual_meas_std, MH_thresh, initial_std_x / _y / _z, Qimu.gyro / .accel / .gyro_bias / .accel_bias, "
                         "Qmodel.Wsb / .Wbc / .Wsg")
    ap.add_argument("-worlds", type=int, default=16, help="shared worlds W: every tuning runs on the same W sequences")
    ap.add_argument("-total_time", type=float, default=4.0)
    ap.add_argument("-imu_dt", type=float, default=0.0025)
    ap.add_argument("-vision_dt", type=float, default=0.04)
    ap.add_argument("-noise_vision_std", type=float, default=1.0)
    ap.add_argument("-npts", type=int, default=1000)
    ap.add_argument("-seed", type=int, default=0)
    ap.add_argument("-feature_init", default="immediate", choices=["immediate", "subfilter"],
                    help="the device life cycle the sweep runs on: lifecycle='device' or, for subfilter, pool_lifecycle='device'")
    ap.add_argument("-tracks", default="host", choices=["host", "device"],
                    help="host (default): the numpy worlds' tracks, uploaded and tiled; device: the worlds tiled on the device, the "
                         "producer's streams shared between the tunings (xivo_hip_pcw_stream_share)")
    ap.add_argument("-noise-seed", dest="noise_seed", type=int, default=0,
                    help="-tracks device: the key of the producer's generator (pixel noise and track faults)")
    # track faults of the device producer (xivo_hip_pcw_fault_config), the options of scripts/run_pcw.py; they need -tracks device
    ap.add_argument("-drop-prob", dest="drop_prob", type=float, default=0.0,
                    help="track faults: the chance per visible point and frame that its track is lost")
    ap.add_argument("-outlier-prob", dest="outlier_prob", type=float, default=0.0, help="track faults: the chance of a gross outlier")
    ap.add_argument("-outlier-px", dest="outlier_px", type=float, nargs=2, default=[20.0, 60.0], metavar=("MIN", "MAX"),
                    help="track faults: each component of an outlier's offset is +-[MIN, MAX] px")
    ap.add_argument("-outlier-sticky", dest="outlier_sticky", action="store_true",
                    help="track faults: an outlier's offset stays on the track until the track ends (default: one frame)")
    ap.add_argument("-tail-prob", dest="tail_prob", type=float, default=0.0,
                    help="track faults: the chance of a heavy-tailed pixel noise draw")
    ap.add_argument("-tail-scale", dest="tail_scale", type=float, default=4.0,
                    help="track faults: a tail draw multiplies noise_vision_std by this")
    ap.add_argument("-out", default="", metavar="FILE.json", help="also write the JSON there")
    return ap


def axes_of(args):
    axes = OrderedDict()
    for name, values in args.axis:
        if name in axes:
            raise ValueError("axis %s is given twice" % name)
        axes[name] = values
    return axes


def best_rows(summary):
    """the index of the best tuning by median aligned ATE and by |nis_per_dof - 1| (None when no row has a finite value)"""
    def arg(v):
        v = np.asarray(v, dtype=float)
        return int(np.nanargmin(v)) if np.isfinite(v).any() else None
    return {"ate_aligned_m": arg([r["ate_aligned_m"] for r in summary]),
            "nis_per_dof": arg([abs(r["nis_per_dof"] - 1.0) for r in summary])}


def main(argv=None):
    args = make_parser().parse_args(argv)
    from xivo_amd import sequence, sweep
    axes = axes_of(args)
    kw = dict(feature_init="subfilter", pool_lifecycle="device") if args.feature_init == "subfilter" else dict(lifecycle="device")
    if args.drop_prob or args.outlier_prob or args.tail_prob or args.outlier_sticky:
        if args.tracks != "device":
            raise SystemExit("the track-fault options need -tracks device: host tracks are not scored")
        kw["track_faults"] = dict(sticky=int(args.outlier_sticky), p_drop=args.drop_prob, p_outlier=args.outlier_prob,
                                  p_tail=args.tail_prob, outlier_min_px=args.outlier_px[0], outlier_max_px=args.outlier_px[1],
                                  tail_scale=args.tail_scale)
    if args.tracks == "device":      # a world never brings more tracks than it has points
        kw["tracks_max"] = max(sequence.SequenceConfig().tracks_max, min(args.npts, sequence.L.LIFE_MAX_TRACKS))
    cfg = sequence.SequenceConfig(**kw)
    timers = {}
    t0 = time.perf_counter()
    out = sweep.run_sweep(cfg, axes, args.worlds, total_time=args.total_time, imu_dt=args.imu_dt, vision_dt=args.vision_dt,
                          noise_vision_std=args.noise_vision_std, npts=args.npts, seed=args.seed, timers=timers,
                          track_source=args.tracks, noise_seed=args.noise_seed)
    wall = time.perf_counter() - t0
    names = list(axes)
    table = []
    for t, row in enumerate(out["summary"]):
        rec = {"tuning": t}
        rec.update({n: (getattr(out["cfgs"][t], n.split(".")[0])[n.split(".")[1]] if "." in n else getattr(out["cfgs"][t], n))
                    for n in names})
        rec.update(row)
        if "outlier_rejected" in row:     # track faults: the gate's detection and false-alarm rates of the tuning
            n_out, n_nom = row["outlier_rejected"] + row["outlier_kept"], row["nominal_rejected"] + row["nominal_kept"]
            rec["detection_rate"] = row["outlier_rejected"] / n_out if n_out else None
            rec["false_alarm_rate"] = row["nominal_rejected"] / n_nom if n_nom else None
        table.append(rec)
    best = best_rows(out["summary"])
    rep = {"axes": out["axes"], "tunings": out["T"], "worlds": out["W"], "filters": out["T"] * out["W"], "frames": out["frames"],
           "contexts": 1, "runs": 1, "tracks": args.tracks, "wall_s": wall, "frame_ms": 1e3 * timers.get("frame", 0.0) / max(out["frames"], 1),
           "table": table, "best": {k: (table[i] if i is not None else None) for k, i in best.items()}}
    line = json.dumps(rep)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return rep


if __name__ == "__main__":
    main()
