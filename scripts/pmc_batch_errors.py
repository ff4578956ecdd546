"""Workload for the FETCH_SIZE counter run of the batched error block (profiles/batch_pmc_fetch_summary.txt): 20000 x 10000, fp32-operand
mode, 8 members of rank 8, 4 iterations with trace 2 (3 error blocks).  The upload kernels of the same run (a16_convert_kernel,
absmax_f32_kernel) stream A exactly once and calibrate what one pass over A reads as on the counter.
Run under: rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR -o batch -- python scripts/pmc_batch_errors.py
then: python scripts/pmc_batch_errors.py --summary DIR/batch_counter_collection.csv"""
import collections
import csv
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def summary(path):
    d = collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        d[r["Kernel_Name"].split("(")[0]].append(float(r["Counter_Value"]))
    one_pass = sum(d["a16_convert_kernel"]) / max(1, len(d["a16_convert_kernel"]))
    print("FETCH_SIZE (KB) per dispatch, averaged per kernel; one pass over A (a16_convert_kernel) = %.0f KB" % one_pass)
    for k, v in sorted(d.items(), key=lambda t: -max(t[1])):
        avg = sum(v) / len(v)
        print(f"{k:45s} dispatches={len(v):4d}  FETCH_SIZE_KB_avg={avg:12.1f}  passes_of_A={avg / one_pass:6.3f}")


def main():
    import nnlm_amd
    from nnlm_amd import _lib
    n, m = 20000, 10000
    rng = np.random.default_rng(0)
    A = np.asfortranarray(rng.random((n, 10)) @ rng.random((10, m)) + 0.1 * rng.random((n, m)))
    ks = [8] * 8
    inits = [(0.01 * rng.random((n, k)), 0.01 * rng.random((k, m))) for k in ks]
    z = [0.0] * 3
    with nnlm_amd.Handle(0, _lib.PREC_F32) as h:
        h.set_matrix(A)
        h.set_factors_batch(ks, [w for w, _ in inits], [x for _, x in inits])
        t = h.run_batch(z, z, 4, -1.0, 0, False, 50, 1e-9, 1, 2)
        print("error blocks:", len(t[0]["mse_error"]))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--summary":
        summary(sys.argv[2])
    else:
        main()
