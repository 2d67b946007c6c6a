#!/usr/bin/env python3
"""Generate tests/golden/separation_queries.npz: the query families of tests/separation_cases.py (seven far families of 150, four
near-contact families of 250 / 250 / 100 / 100, fixed seeds) with the certified bracket (lo, up) of every query's distance.  The
near-contact queries are placed by bisection on the reference itself, about half a second each, which is why they are committed
rather than drawn by every test run.  CPU only:

    python tests/golden/gen_separation_queries.py

Afterwards the script runs the oracle over the set and prints the table by family and exit and the oracle's largest excess over the
reference's upper bound -- the measurement behind separation_cases.ORACLE_MAX_EXCESS (SLIVER_CAP is twice that); DESIGN.md section 3
records it.
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import separation_cases as sc
    from oracle import binding as oracle

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=sc.FIXTURE)
    args = ap.parse_args()
    t0 = time.time()
    cases = sc.generate_queries()
    brackets = np.array([sc.exact_separation(q) for _, q in cases])
    print(f"{len(cases)} queries in {time.time() - t0:.0f} s; widest bracket {np.max(brackets[:, 1] - brackets[:, 0]):.2e}, "
          f"dropped (wider than {sc.BRACKET_CAP:g}): {int((~sc.kept(brackets[:, 0], brackets[:, 1])).sum())}")
    sc.save_fixture(args.out, cases, brackets)
    size = os.path.getsize(args.out)
    print(args.out, size, "bytes")
    assert size <= 500_000, "the fixture is to stay below 500 KB"
    cases, lo, up = sc.load_fixture(args.out)
    oracle.build()
    rows = sc.oracle_rows(oracle, cases)
    print("\n".join(sc.census_table(rows, lo, up)))
    d = np.array([r["distance"] for r in rows])
    sep = np.array([not r["penetrating"] for r in rows]) & sc.kept(lo, up)
    stable = np.array([r["stable"] for r in rows]) & sep
    print(f"oracle: lowest d - lo {np.min((d - lo)[sep]):+.2e}; largest d - up on the stable set {np.max((d - up)[stable]):+.2e}, "
          f"off it (ORACLE_MAX_EXCESS) {np.max((d - up)[sep & ~stable]):.4e}")


if __name__ == "__main__":
    main()
