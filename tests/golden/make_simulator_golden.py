#!/usr/bin/env python3
"""Regenerate tests/golden/simulator_expected.json from the REFERENCE RFISimulator (rfi_toolbox/core/simulator.py).

    python tests/golden/make_simulator_golden.py /path/to/reference_checkout

The reference is pure NumPy; this runs it on the host with its own global random stream:
  - deterministic pieces, pinned bitwise (float.hex): _make_gibbs_kernel() and _phase_grid on fixed parameters;
  - distribution statistics (tests/rfisim_ref.py: sample_stats / clean_stats) over SEEDS seeds at 256x256 and
    128x384, ringing off and on, each as the mean and standard deviation across seeds;
  - the reference's CPU time for one generate_rfi() at 1024x1024 on the machine that ran this script (median of
    three, single process), quoted by tools/bench_rfi_simulator.py.
"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from rfisim_ref import aggregate, clean_stats, sample_stats   # noqa: E402

SEEDS = 24
SHAPES = ((256, 256), (128, 384))
PHASE_PARAMS = ((0.013, 0.0, -0.021, 1.25), (-0.11, 3.0e-4, 0.0071, 5.5))


def planes_of(tf):
    return np.stack([tf[p] for p in ("RR", "RL", "LR", "LL")])


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from rfi_toolbox.core.simulator import RFISimulator

    out = {"generator": "tests/golden/make_simulator_golden.py", "seeds": SEEDS}
    k = RFISimulator._make_gibbs_kernel()
    out["gibbs_kernel_hex"] = [float(v).hex() for v in k]
    t = np.arange(7)[:, None]
    n = np.arange(5, 12)[None, :]
    out["phase_grid"] = [{"params": list(p), "t": "arange(7)[:, None]", "n": "arange(5, 12)[None, :]",
                          "hex": [float(v).hex() for v in RFISimulator._phase_grid(t, n, p).ravel()]}
                         for p in PHASE_PARAMS]
    stats = {}
    for T, F in SHAPES:
        for ring in (False, True):
            per = []
            for seed in range(SEEDS):
                np.random.seed(1000 + seed)
                sim = RFISimulator(T, F)
                sim.gibbs_ringing = ring
                tf, mask = sim.generate_rfi()
                per.append(sample_stats(planes_of(tf), mask))
            stats[f"{T}x{F}_ring{int(ring)}"] = aggregate(per)
        per = []
        for seed in range(SEEDS):
            np.random.seed(2000 + seed)
            tf, _ = RFISimulator(T, F).generate_clean_data()
            per.append(clean_stats(planes_of(tf)))
        stats[f"{T}x{F}_clean"] = aggregate(per)
    out["stats"] = stats
    times = []
    for seed in range(3):
        np.random.seed(seed)
        sim = RFISimulator(1024, 1024)
        t0 = time.process_time()
        sim.generate_rfi()
        times.append(time.process_time() - t0)
    out["reference_cpu_seconds_1024x1024"] = {"median": float(np.median(times)), "runs": times,
                                              "note": "one generate_rfi() on one CPU core of the development host"}
    with open(os.path.join(HERE, "simulator_expected.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
