"""Diagnosis aid for tests/test_gpu_fuzz.py (run on the GPU box: python tests/fuzz_table.py): one line per failing or degenerate case of the
first NNLM_FUZZ_SEEDS (default 150) seeds of both modes -- deviations of W and H, iteration and sweep counts, the case's parameters.
--sparse: the same for the whole-run cases of tests/test_gpu_fuzz_sparse.py (sparse_cases.make_case under both semantics).
--families: one line per case of tests/test_gpu_data_families.py (data_cases.cases(), the dup and the exact_state cases), both modes, with the
oracle's own deviation between two summation orders beside the deviations of W and H."""
import os, sys
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE))
import test_gpu_fuzz as F
from helpers import relF
if "--sparse" in sys.argv:
    import sparse_cases as sc
    import test_gpu_fuzz_sparse as S
    from oracle import ref
    for mode in ("f64", "f32"):
        os.environ["NNLM_PRECISION"] = mode
        tol = 1e-9 if mode == "f64" else 1e-4
        for semantics in sc.SEMANTICS:
            for seed in range(int(os.environ.get("NNLM_FUZZ_SEEDS", "150"))):
                c = sc.make_case(seed, semantics)
                try:
                    r, o = S.run_both(c)
                except Exception as e:
                    print(mode, semantics, seed, "EXC", repr(e)[:200], sc.describe(c)); continue
                ew, eh = relF(r["W"], o["W"]), relF(r["H"], o["H"])
                ep = np.array_equal(r["average_epoch"], o["average_epoch"]) if r["average_epoch"].shape == o["average_epoch"].shape else "shape"
                deg = sc.degenerate(c, ref)
                if deg or not (ew < tol and eh < tol) or r["n_iteration"] != o["n_iteration"] or (mode == "f64" and ep is not True):
                    print(mode, semantics, seed, "DEG" if deg else "   ", "LOOSE" if sc.rank_deficient(c) else "     ",
                          f"W {ew:.2e} H {eh:.2e} nit {r['n_iteration']}/{o['n_iteration']} ep_eq {ep}", sc.describe(c), flush=True)
    sys.exit(0)
if "--families" in sys.argv:
    import data_cases as dc
    import nnlm_amd
    from oracle import ref
    runs = [(dc.case_id(t), dc.make_case(*t)) for t in dc.cases()]
    runs += [(f"dup-{sh[0]}x{sh[1]}k{sh[2]}-m{me}-na{int(na)}", dc.make_dup_case(sh, me, na)) for sh in dc.SHAPES for me in dc.METHODS for na in (False, True)]
    runs += [(f"exact_state-m{me}", dc.make_exact_state_case(me)) for me in (3, 4)]
    for name, c in runs:
        o, orev = dc.oracle_runs(c)
        wp = dc.well_posed_deviation(c, key=name)
        for mode in ("f64", "f32"):
            os.environ["NNLM_PRECISION"] = mode
            tol = 1e-9 if mode == "f64" else 1e-4
            try:
                r = nnlm_amd.c_nnmf(*dc.nnmf_args(c))
            except Exception as e:
                print(mode, name, "EXC", repr(e)[:200], dc.describe(c)); continue
            ew, eh = relF(r["W"], o["W"]), relF(r["H"], o["H"])
            ep = np.array_equal(r["average_epoch"], o["average_epoch"]) if r["average_epoch"].shape == o["average_epoch"].shape else "shape"
            lost = int(((r["W"] == 0) & (o["W"] > 0)).sum() + ((r["H"] == 0) & (o["H"] > 0)).sum())
            print(mode, name, "   " if ew < tol and eh < tol else "BAD", f"W {ew:.2e} H {eh:.2e} oracle {wp:.1e} nit {r['n_iteration']}/{o['n_iteration']} ep_eq {ep} "
                  f"oracle_ep_eq {np.array_equal(o['average_epoch'], orev['average_epoch'])} lost {lost}", flush=True)
    sys.exit(0)
HARD = os.environ.get("NNLM_FUZZ_F32_HARD", "0") == "1"  # F32 mode on the strict mode's cases too (ranks up to the smaller dimension, up to 90 % missing)
for mode, wc in (("f64", False), ("f32", not HARD)):
    os.environ["NNLM_PRECISION"] = mode
    tol = 1e-9 if mode == "f64" else 1e-4
    for seed in range(int(os.environ.get("NNLM_FUZZ_SEEDS", "150"))):
        c = F.make_case(seed, wc)
        try:
            r, o = F.run_both(c)
        except Exception as e:
            print(mode, seed, "EXC", repr(e)[:200], F.describe(c)); continue
        ew, eh = relF(r["W"], o["W"]), relF(r["H"], o["H"])
        ep = np.array_equal(r["average_epoch"], o["average_epoch"]) if r["average_epoch"].shape == o["average_epoch"].shape else "shape"
        deg = F.degenerate(c)
        bad = not (ew < tol and eh < tol) or r["n_iteration"] != o["n_iteration"] or (mode == "f64" and ep is not True)
        if bad:
            d = F.describe(c)
            print(mode, seed, "DEG" if deg else "   ", f"W {ew:.2e} H {eh:.2e} nit {r['n_iteration']}/{o['n_iteration']} ep_eq {ep}", d["shape"], "k", d["k"], "meth", d["method"], f"na {d['na']:.2f}", "masks", d["masks"], "a", d["alpha"], "b", d["beta"], "it", d["max_iter"], "tr", d["trace"], "inner", d["inner"], flush=True)
