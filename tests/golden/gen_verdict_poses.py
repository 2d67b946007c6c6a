#!/usr/bin/env python3
"""Generate tests/golden/verdict_poses.npz: arm poses in which ONE check_collision pair sits at a prescribed signed gap from the
0.01 m contact margin and the other 23 pairs are certified free (tests/verdict_cases.py states the pair list and the rule).  CPU only:

    python tests/golden/gen_verdict_poses.py [--jobs 16]

  directed family   per pair and gap of verdict_cases.GAPS, POSES_PER_CELL poses.  Table, track and self pairs: a random q, one joint
                    moved until the pair's distance is margin + gap.  Obstacle pairs: a random free q, the cylinder slid along a random
                    line through the link's centroid (as separation_cases.refresh_near_state does).
  tight family      table and track pairs at the margin, the TIGHT_COUNT poses in which the bounding-capsule bound of the culling pass is
                    least conservative (certified hull distance minus capsule bound) among at least 5000 candidates.

The ORACLE steers: it finds near poses, scans a joint for a crossing of the margin and checks isolation first, because it is fast.
Only the reference certifies: every committed pose is placed by a root search on separation_cases.core_bracket's own upper bound,
and carries the reference's (lo, up) of its pair and the smallest lo of the others; a bracket wider than BRACKET_CAP is not committed.
Fixed seeds, one stream per pair: the output does not depend on --jobs.

A pair for which the budget runs out is reported with the smallest distance it reached with the others isolated (by the oracle) and
must stand in verdict_cases.UNREACHED; DESIGN.md section 3 records the table this script prints.
"""
import argparse
import multiprocessing as mp
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import separation_cases as sc  # noqa: E402
import verdict_cases as vc  # noqa: E402
from oracle import binding as oracle  # noqa: E402

BUDGET = 200_000          # steered candidates (random q drawn and judged by the oracle) before a pair is given up
NEAR = 0.015              # a candidate is scanned when its pair is this close
SCAN_HALF, SCAN_POINTS = 0.5, 17
PRE_ISOLATION = 1.5e-3    # the oracle's filter on the other pairs at the crossing (the certificate asks ISOLATION of the reference)
TIGHT_CANDIDATES, TIGHT_CHUNKS = 5120, 16
M = vc.M

_BOXES = ((oracle.BOX, sc.TABLE_HALF, sc.TABLE_POSE), (oracle.BOX, sc.TRACK_HALF, sc.TRACK_POSE))


def oracle_pairs(q, obst, only=None):
    """The oracle's distance of the 24 pairs (inf where not asked)."""
    rot, pos = oracle.fk(q)
    pose = {}
    out = np.full(vc.N_PAIRS, np.inf)
    for k, (a, b) in enumerate(vc.PAIRS):
        if only is not None and k not in only:
            continue
        for l in (a, b):
            if not isinstance(l, str) and l not in pose:
                pose[l] = np.r_[pos[l], sc.matrix_to_quat(rot[l])]
        if a == "obstacle":
            other = (oracle.CYLZ, sc.CYL[:2], obst)
        elif isinstance(a, str):
            other = _BOXES[a == "track"]
        else:
            other = (oracle.HULL, [a], pose[a])
        out[k] = oracle.closest(oracle.HULL, [b], pose[b], *other)["distance"]
    return out


def draw_q(rng):
    q = rng.uniform(-np.pi, np.pi, 6)
    if rng.random() < 0.75:
        q[1] = rng.uniform(-np.pi, 0.0)  # shoulder mostly above the table, as in test_collision_verdict_census
    return q


def joints_of(pair):
    a, b = vc.PAIRS[pair]
    return list(range(0 if isinstance(a, str) else a, b))  # the joints between the two bodies (0-based): they move the pair's distance


def root_search(f, x0, x1, f0, f1):
    """Illinois search for f = 0 in [x0, x1], f0 <= 0 < f1; ends at |f| <= GAP_TOL / 10 or neighbouring arguments."""
    side = 0
    for _ in range(200):
        x = x1 - f1 * (x1 - x0) / (f1 - f0)
        if not x0 < x < x1:
            x = 0.5 * (x0 + x1)
        if x == x0 or x == x1:
            break
        fx = f(x)
        if abs(fx) <= 0.1 * vc.GAP_TOL:
            return x
        if fx > 0.0:
            x1, f1 = x, fx
            if side == 1:
                f0 *= 0.5
            side = 1
        else:
            x0, f0 = x, fx
            if side == -1:
                f1 *= 0.5
            side = -1
    return x1 if abs(f1) <= abs(f0) else x0


def golden_min(f, a, b, evals=30):
    """Golden-section search for the lowest point of f on [a, b]."""
    g = 0.5 * (np.sqrt(5.0) - 1.0)
    c, d = b - g * (b - a), a + g * (b - a)
    fc, fd = f(c), f(d)
    for _ in range(evals):
        if fc < fd:
            b, d, fd = d, c, fc
            c = b - g * (b - a)
            fc = f(c)
        else:
            a, c, fc = c, d, fd
            d = a + g * (b - a)
            fd = f(d)
    return c if fc < fd else d


def steer(q, pair, rng, steps=15):
    """Hill climb (oracle) on all six joints towards poses in which `pair` is the closest pair by far: lowers the pair's distance
    minus the smallest of the others'.  Returns (q, that difference)."""
    def score(x):
        d = oracle_pairs(x, vc.FAR_OBSTACLE)
        return (d[pair] - np.delete(d, pair).min()) if d[pair] < 2.0 * NEAR else np.inf

    best = score(q)
    for k in range(steps):
        x = q + rng.normal(0.0, 0.3 * 0.9 ** k, 6)
        x = np.clip(x, -np.pi, np.pi)
        sx = score(x)
        if sx < best:
            q, best = x, sx
    return q, best


def certify(q, obst, pair, gap, family):
    """The committed row of a placed pose, or None with the reason."""
    lo, up = vc.pair_brackets(q, obst, only=(pair,))
    if up[pair] - lo[pair] > vc.BRACKET_CAP:
        return None, "bracket"
    if abs(up[pair] - (M + gap)) > 0.5 * vc.GAP_TOL:
        return None, "gap"
    others = [k for k in range(vc.N_PAIRS) if k != pair]
    olo, _ = vc.pair_brackets(q, obst, decide=M + 2.0 * vc.ISOLATION, only=others)
    if not (np.delete(olo, pair) > M + vc.ISOLATION).all():
        return None, "isolation"
    # (decide ends a search once lo is past the line: the figure committed is a certified lower bound, not the distance)
    return dict(q=q, obst=obst, pair=pair, gap=gap, family=family, lo=lo[pair], up=up[pair], others_lo=float(np.delete(olo, pair).min())), ""


def place(pose_of, pair, x_cross, gap, x_min, x_max):
    """The argument x near x_cross at which the REFERENCE's distance of `pair` is M + gap: a window grown around the oracle's crossing
    until the reference's values straddle the target, then the root search."""
    def f(x):
        q, obst = pose_of(x)
        return vc.pair_brackets(q, obst, only=(pair,))[1][pair] - (M + gap)

    fc = f(x_cross)
    step = 1e-3
    while step < 1.0:
        xa, xb = max(x_min, x_cross - step), min(x_max, x_cross + step)
        fa, fb = f(xa), f(xb)
        for (u, fu), (v, fv) in (((xa, fa), (x_cross, fc)), ((x_cross, fc), (xb, fb))):
            if fu <= 0.0 < fv:
                return root_search(f, u, v, fu, fv)
            if fv <= 0.0 < fu:
                return root_search(lambda x: -f(x), u, v, -fu, -fv) if fv < 0.0 else v
        step *= 3.0
    if fc > 0.0:
        # the target lies below everything the windows saw (a pair that barely reaches it): the lowest point to either side
        for u, v in ((max(x_min, x_cross - 0.5), x_cross), (x_cross, min(x_max, x_cross + 0.5))):
            xm = golden_min(f, u, v)
            fm = f(xm)
            if fm <= 0.0:
                return root_search(f, xm, x_cross, fm, fc) if xm < x_cross else root_search(lambda x: -f(x), x_cross, xm, -fc, -fm) if fm < 0.0 else xm
    return None


def crossings(pose_of, pair, xs):
    """Scan the oracle's distance of `pair` over xs; for every change of side of the margin, bisect it (oracle) to 1e-7.  Yields x."""
    d = np.array([oracle_pairs(*pose_of(x), only=(pair,))[pair] for x in xs])
    for i in np.nonzero((d[:-1] - M) * (d[1:] - M) < 0.0)[0]:
        a, b, below = xs[i], xs[i + 1], d[i] < M
        for _ in range(40):
            mid = 0.5 * (a + b)
            if (oracle_pairs(*pose_of(mid), only=(pair,))[pair] < M) == below:
                a = mid
            else:
                b = mid
            if abs(b - a) < 1e-7:
                break
        yield 0.5 * (a + b), d


def joint_candidates(pair, rng, budget, want):
    """Steered search for a table / track / self pair: yields (pose_of, x_cross, x_min, x_max); keeps the statistics in `want`."""
    joints = joints_of(pair)
    while want["candidates"] < budget:
        q = draw_q(rng)
        want["candidates"] += 1
        d = oracle_pairs(q, vc.FAR_OBSTACLE, only=(pair,))[pair]
        if d < want["closest"]:
            want["closest"] = d
        if d > NEAR:
            continue
        scan = [joints[int(rng.integers(len(joints)))]]
        if rng.random() < 0.1:  # every tenth near candidate is steered first, and then every joint of the pair is scanned
            q, lead = steer(q, pair, rng)
            want["steered"] = want.get("steered", 0) + 1
            if lead > 0.0:
                continue
            scan = joints
        for j in scan:
            def pose_of(x, q=q, j=j):
                qq = q.copy()
                qq[j] = x
                return qq, vc.FAR_OBSTACLE

            lo_x, hi_x = max(-np.pi, q[j] - SCAN_HALF), min(np.pi, q[j] + SCAN_HALF)
            for x, d in crossings(pose_of, pair, np.linspace(lo_x, hi_x, SCAN_POINTS)):
                if d.min() > M + min(vc.GAPS) + 1e-3:
                    continue  # (the scan never comes near the deepest gap: not a base)
                others = np.delete(oracle_pairs(*pose_of(x)), pair)
                if others.min() > M + vc.ISOLATION:
                    want["isolated"] = min(want["isolated"], M)
                if others.min() > M + PRE_ISOLATION:
                    yield pose_of, x, lo_x, hi_x


def obstacle_candidates(pair, rng, budget, want):
    """Steered search for an obstacle pair: a free q, the cylinder slid along a random line through the link's centroid."""
    link = vc.PAIRS[pair][1]
    arm = list(range(vc.N_OBST, vc.N_PAIRS))
    while want["candidates"] < budget:
        q = np.r_[rng.uniform(-np.pi, np.pi), rng.uniform(-2.2, -0.4), rng.uniform(-2, 2, 4)]
        want["candidates"] += 1
        if oracle_pairs(q, vc.FAR_OBSTACLE, only=arm).min() < M + 5e-3:
            continue
        R, t = sc.numpy_fk(q)
        anchor = (sc.hull_verts(link) @ R[link].T + t[link]).mean(0)
        quat = sc.matrix_to_quat(sc._rpy_matrix(np.r_[rng.uniform(-2.6, 2.6, 2), 0.0]))
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)

        def pose_of(s, q=q, anchor=anchor, d=d, quat=quat):
            return q, np.r_[anchor + s * d, quat]

        for x, dist in crossings(pose_of, pair, np.linspace(0.0, 0.8, SCAN_POINTS)):
            want["closest"] = min(want["closest"], float(dist.min()))
            others = np.delete(oracle_pairs(*pose_of(x)), pair)
            if others.min() > M + vc.ISOLATION:
                want["isolated"] = min(want["isolated"], M)
            if others.min() > M + PRE_ISOLATION:
                yield pose_of, x, 0.0, 2.0


def directed(pair):
    """POSES_PER_CELL bases of one pair, each placed at every gap: (rows, statistics)."""
    rng = np.random.default_rng(7000 + pair)
    want = dict(pair=pair, candidates=0, closest=np.inf, isolated=np.inf, bases=0, rejected={})
    gen = (obstacle_candidates if pair < vc.N_OBST else joint_candidates)(pair, rng, BUDGET, want)
    rows = []
    for pose_of, x, x_min, x_max in gen:
        base = []
        for gap in vc.GAPS:
            xg = place(pose_of, pair, x, gap, x_min, x_max)
            row, why = (None, "window") if xg is None else certify(*pose_of(xg), pair, gap, vc.FAMILY_DIRECTED)
            if row is None:
                want["rejected"][why] = want["rejected"].get(why, 0) + 1
                break
            base.append(row)
        if len(base) == len(vc.GAPS):
            rows += base
            want["bases"] += 1
            if want["bases"] == vc.POSES_PER_CELL:
                break
    return rows, want


def capsule_bound(lib, q, pair):
    return vc.cull_masks(lib, q, M)[2][0, pair - vc.N_OBST]


def tight_chunk(chunk):
    """TIGHT_CANDIDATES / TIGHT_CHUNKS crossings of table and track pairs (oracle), each with its conservatism: the oracle's distance
    at the crossing minus the capsule bound of the culling pass."""
    rng = np.random.default_rng(9000 + chunk)
    lib = vc.build_harness()
    pairs = [k for k in range(vc.N_OBST, vc.N_OBST + 10) if vc.PAIR_NAMES[k] not in vc.UNREACHED]
    out = []
    while len(out) < TIGHT_CANDIDATES // TIGHT_CHUNKS:
        pair = pairs[int(rng.integers(len(pairs)))]
        want = dict(candidates=0, closest=np.inf, isolated=np.inf)
        for pose_of, x, x_min, x_max in joint_candidates(pair, rng, 2000, want):
            q = pose_of(x)[0]
            out.append((M - capsule_bound(lib, q, pair), pair, q, x, x_min, x_max))
            break
    return out


def tight_rows(cands):
    """The TIGHT_COUNT least conservative candidates that the reference can place and certify, at the gaps TIGHT_GAPS in turn."""
    lib = vc.build_harness()
    rows, worst = [], []
    for cons, pair, q, x, x_min, x_max in sorted(cands, key=lambda c: c[0]):
        joint = next(k for k in joints_of(pair) if q[k] == x)  # (the joint the candidate's scan moved: pose_of put x there)

        def pose_of(v, q=q, joint=joint):
            qq = q.copy()
            qq[joint] = v
            return qq, vc.FAR_OBSTACLE

        gap = vc.TIGHT_GAPS[len(rows) % len(vc.TIGHT_GAPS)]
        xg = place(pose_of, pair, x, gap, x_min, x_max)
        if xg is None:
            continue
        row, _ = certify(*pose_of(xg), pair, gap, vc.FAMILY_TIGHT)
        if row is None:
            continue
        rows.append(row)
        worst.append(row["up"] - capsule_bound(lib, row["q"], pair))
        if len(rows) == vc.TIGHT_COUNT:
            break
    return rows, worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=vc.FIXTURE)
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    args = ap.parse_args()
    oracle.build()
    vc.build_harness()
    t0 = time.time()
    with mp.Pool(args.jobs) as pool:
        results = pool.map(directed, range(vc.N_PAIRS), chunksize=1)
        cands = [c for part in pool.map(tight_chunk, range(TIGHT_CHUNKS), chunksize=1) for c in part]
    rows = [r for part, _ in results for r in part]
    print(f"directed family: {len(rows)} poses in {time.time() - t0:.0f} s; budget {BUDGET} steered candidates per pair")
    print("  pair            bases  candidates  closest (oracle)  rejected bases")
    unreached = []
    for _, w in results:
        name = vc.PAIR_NAMES[w["pair"]]
        note = ""
        if w["bases"] < vc.POSES_PER_CELL:
            unreached.append(name)
            note = f"  UNREACHED: smallest distance {w['closest']:.4f} m" + ("" if np.isfinite(w["isolated"]) else ", never at the margin with the others free")
        print(f"  {name:14s} {w['bases']:5d} {w['candidates']:11d} {w['closest']:17.4f}  {w['rejected']}{note}")
    trows, cons = tight_rows(cands)
    allc = np.array([c[0] for c in cands])
    print(f"tight family: {len(cands)} candidates at the margin (table and track pairs); conservatism of the capsule bound over them: "
          f"smallest {allc.min():.3e}, median {np.median(allc):.3e} m")
    print(f"  {len(trows)} committed; certified hull distance minus capsule bound: smallest {min(cons):.3e}, largest {max(cons):.3e} m; pairs "
          + ", ".join(sorted({vc.PAIR_NAMES[r['pair']] for r in trows})))
    assert len(trows) == vc.TIGHT_COUNT and len(cands) >= 5000
    rows += trows
    width = max(r["up"] - r["lo"] for r in rows)
    print(f"{len(rows)} poses; widest bracket {width:.2e}; smallest isolation of the others {min(r['others_lo'] for r in rows) - M:.2e} above the margin")
    vc.save_fixture(args.out, rows)
    size = os.path.getsize(args.out)
    print(args.out, size, "bytes")
    assert size <= 500_000, "the fixture is to stay below 500 KB"
    assert sorted(unreached) == sorted(vc.UNREACHED), (unreached, "verdict_cases.UNREACHED must list exactly these")
    assert len(unreached) <= 4


if __name__ == "__main__":
    main()
