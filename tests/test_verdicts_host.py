"""Host tests (-m "not gpu") of the collision verdict's path against the certified brackets of tests/separation_cases.py, through
tests/verdict_cases.py (the pair list and the rule) and tests/verdict_harness.cpp (the culling pass of urgym_hip.hip P1 with the
bounds of urgym_device.h, compiled with g++):

  a  every hull vertex lies inside its link's bounding capsule; the table of data/ur5e_model.h is the model file's, bit for bit
  b  seg_box_lower_bound2 and segseg_dist2 are lower bounds of the distance between the vertex sets (a segment is 2 points, a box 8
     corners): bound <= up + LD_TOL, in the families where such formulas go wrong
  c  no culled pair is in contact: on the committed poses and 2000 random ones, at margins 0.01, 0 and 0.05, every pair either form
     of the predicate drops whose capsule bound is within 2 cm of the reach is certified lo > margin
  d  the fixture says what it claims (a seeded sample re-certified from scratch) and the ORACLE's verdict on every committed pose obeys
     the rule
  e  coverage: every pair outside verdict_cases.UNREACHED has every gap; the tight family is there
Run with -s for the figures (DESIGN.md section 3 quotes them).
"""
import numpy as np
import pytest

import separation_cases as sc
import verdict_cases as vc

M = vc.M


@pytest.fixture(scope="module")
def lib():
    return vc.build_harness()


@pytest.fixture(scope="module")
def fx():
    return vc.load_fixture()


# ------------------------------------------------------------------------------------------------ a: containment
def _segment_distance(v, p0, p1):
    d = p1 - p0
    u = np.clip(((v - p0) @ d) / (d @ d), 0.0, 1.0)
    return np.sqrt((((v - p0) - u[:, None] * d) ** 2).sum(1))


def test_capsules_contain_their_hulls(lib):
    tab = vc.capsule_table(lib)
    npz = np.c_[sc.MODEL["capsule_p0"], sc.MODEL["capsule_p1"], sc.MODEL["capsule_r"]]
    assert tab.shape == npz.shape and np.array_equal(tab.view(np.int64), npz.view(np.int64)), "ur5e_model.h and ur5e_model.npz differ"
    print()
    for link in range(1, 7):
        c = tab[link - 1]
        dist = _segment_distance(sc.hull_verts(link), c[:3], c[3:6])
        slack = c[6] - dist
        print(f"  link {link}: {len(dist)} vertices, radius {c[6]:.6f}, smallest slack {slack.min():.3e} m, {int((slack < 1.1e-9).sum())} vertices within 1.1e-9 of the surface")
        assert (dist <= c[6]).all(), (link, "a vertex outside its capsule by", -slack.min())


# ------------------------------------------------------------------------------------------------ b: the two bounds
def _points_core(pts):
    c = sc.Core(sc.SPHERE, [0.0], np.r_[0.0, 0.0, 0.0, 0, 0, 0, 1.0])
    c.verts = np.asarray(pts, np.float64).reshape(-1, 3)
    c.t = c.verts.mean(0)
    return c


def _box_core(box):
    return _points_core(box[:3] + sc._CORNERS * box[3:])


def seg_box_families(rng, per=340):
    """{family: (seg [n, 6], box [n, 6])}."""
    fam = {}
    rbox = lambda n: np.c_[rng.uniform(-0.5, 0.5, (n, 3)), rng.uniform(0.02, 0.9, (n, 3))]

    def add(name, seg, box):
        fam[name] = (np.asarray(seg, np.float64).reshape(-1, 6), box)

    n = per
    box = rbox(n)                                   # parallel to a face (one coordinate fixed) or an edge (two fixed), outside at a small or large gap
    seg = np.zeros((n, 6))
    for i in range(n):
        c, h = box[i, :3], box[i, 3:]
        p = c + rng.uniform(-1.5, 1.5, 3) * h
        q = c + rng.uniform(-1.5, 1.5, 3) * h
        fixed = rng.permutation(3)[: 1 + i % 2]
        for ax in fixed:
            off = h[ax] + (0.0 if i % 7 == 0 else 10.0 ** rng.uniform(-9, -1))
            p[ax] = q[ax] = c[ax] + rng.choice([-1, 1]) * off
        seg[i] = np.r_[p, q]
    add("parallel to a face or an edge", seg, box)
    box = rbox(n)                                   # through the box: the end points on opposite sides
    s = rng.choice([-1.0, 1.0], (n, 3))
    seg = np.c_[box[:, :3] + s * box[:, 3:] * rng.uniform(1.0, 3.0, (n, 3)), box[:, :3] - s * box[:, 3:] * rng.uniform(1.0, 3.0, (n, 3))]
    add("through the box", seg, box)
    box = rbox(n)                                   # an end point ON a face, an edge or a corner, the other outside
    seg = np.zeros((n, 6))
    for i in range(n):
        c, h = box[i, :3], box[i, 3:]
        on = rng.uniform(-1, 1, 3)
        pin = rng.permutation(3)[: 1 + i % 3]
        sign = rng.choice([-1.0, 1.0], 3)
        on[pin] = sign[pin]
        out = on.copy()
        out[pin] += sign[pin] * rng.uniform(0.0, 2.0, len(pin))
        out += np.where(np.isin(np.arange(3), pin), 0.0, rng.uniform(-1, 1, 3))
        seg[i] = np.r_[c + on * h, c + out * h]
    add("end point on a face, edge or corner", seg, box)
    box = rbox(n)                                   # diagonal past a corner: outside in all three axes at one end, cutting across
    s = rng.choice([-1.0, 1.0], (n, 3))
    a = box[:, :3] + s * box[:, 3:] * (1.0 + 10.0 ** rng.uniform(-6, 0, (n, 3)))
    flip = np.c_[-np.ones(n), np.ones(n), np.ones(n)][:, rng.permutation(3)]
    b = box[:, :3] + s * flip * box[:, 3:] * (1.0 + 10.0 ** rng.uniform(-6, 0.5, (n, 3)))
    add("diagonal past a corner", np.c_[a, b], box)
    box = rbox(n)                                   # degenerate: p == q, anywhere (inside, on, outside)
    p = box[:, :3] + rng.uniform(-2, 2, (n, 3)) * box[:, 3:]
    add("degenerate p == q", np.c_[p, p], box)
    box = np.tile(np.r_[sc.TABLE_POSE[:3], sc.TABLE_HALF], (n, 1))  # the scene's own table with capsule-sized segments just above it
    box[n // 2:] = np.r_[sc.TRACK_POSE[:3], sc.TRACK_HALF]
    p = np.c_[rng.uniform(-0.3, 1.2, n), rng.uniform(-1.0, 1.0, n), box[:, 2] + box[:, 5] + 10.0 ** rng.uniform(-6, -1, n)]
    d = rng.normal(size=(n, 3))
    d[:, 2] = np.abs(d[:, 2]) * rng.choice([0.0, 1e-3, 1.0], n)
    add("capsule-sized, above the table or the track", np.c_[p, p + 0.4 * d / np.linalg.norm(d, axis=1)[:, None]], box)
    return fam


def test_seg_box_bound_is_a_lower_bound(lib):
    fams = seg_box_families(np.random.default_rng(31))
    total = 0
    print()
    for name, (seg, box) in fams.items():
        got = np.sqrt(vc.seg_box_lower_bound2(lib, seg, box))
        br = np.array([sc.core_bracket(_points_core(s), _box_core(b)) for s, b in zip(seg, box)])
        # (up is the norm of a point of A - B whatever the bracket's width: every case is held to it; ok counts the narrow brackets)
        ok = (br[:, 1] - br[:, 0]) <= 1e-9
        excess = got - br[:, 1]
        total += len(seg)
        print(f"  seg<->box {name:44s} {len(seg):4d} cases ({int(ok.sum())} brackets within 1e-9), bound - up: largest {excess.max():+.2e}, "
              f"bound = 0 in {int((got == 0).sum())}, mean conservatism {np.mean(br[:, 1] - got):.2e}")
        assert excess.max() <= sc.LD_TOL, (name, "the bound overstates the distance by", excess.max(), seg[np.argmax(excess)], box[np.argmax(excess)])
    assert total >= 2000


def seg_seg_families(rng, per=260):
    fam = {}
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    rp = lambda n, s=0.5: rng.uniform(-s, s, (n, 3))
    n = per
    c = rp(n)                                       # crossing: the segments meet (or nearly) at an interior point
    d1, d2 = unit(rng.normal(size=(n, 3))), unit(rng.normal(size=(n, 3)))
    off = unit(np.cross(d1, d2)) * (10.0 ** rng.uniform(-12, -2, (n, 1))) * (rng.random((n, 1)) < 0.7)
    fam["crossing"] = (np.c_[c - d1 * rng.uniform(0.05, 0.5, (n, 1)), c + d1 * rng.uniform(0.05, 0.5, (n, 1))],
                       np.c_[c + off - d2 * rng.uniform(0.05, 0.5, (n, 1)), c + off + d2 * rng.uniform(0.05, 0.5, (n, 1))])
    p, d = rp(n), unit(rng.normal(size=(n, 3)))     # collinear: overlapping or apart
    t = np.sort(rng.uniform(-1, 1, (n, 4)), axis=1)
    t = np.where((np.arange(n) % 2 == 0)[:, None], t, t[:, [0, 2, 1, 3]])
    fam["collinear, overlapping or apart"] = (np.c_[p + d * t[:, :1], p + d * t[:, 1:2]], np.c_[p + d * t[:, 2:3], p + d * t[:, 3:4]])
    p, d = rp(n), unit(rng.normal(size=(n, 3)))     # parallel at an offset
    o = unit(np.cross(d, rng.normal(size=(n, 3)))) * 10.0 ** rng.uniform(-8, -0.5, (n, 1))
    t = rng.uniform(-1, 1, (n, 4))
    fam["parallel"] = (np.c_[p + d * t[:, :1], p + d * t[:, 1:2]], np.c_[p + o + d * t[:, 2:3], p + o + d * t[:, 3:4]])
    # near-parallel at angles 1e-4 .. 1e-15: both sides of den > 1e-30 (den = |d1|^2 |d2|^2 sin^2: with lengths 1e-3 .. 1 the branch
    # flips between angle 1e-15 and 1e-9)
    m = 2 * n
    p, d = rp(m), unit(rng.normal(size=(m, 3)))
    perp = unit(np.cross(d, rng.normal(size=(m, 3))))
    ang = 10.0 ** rng.uniform(-15, -4, (m, 1))
    d2 = unit(d + perp * ang)
    l1, l2 = 10.0 ** rng.uniform(-3, 0, (m, 1)), 10.0 ** rng.uniform(-3, 0, (m, 1))
    o = unit(np.cross(d, perp)) * 10.0 ** rng.uniform(-6, -1, (m, 1)) * (rng.random((m, 1)) < 0.8)
    sh = rng.uniform(-1.5, 1.5, (m, 1)) * np.maximum(l1, l2)
    fam["near-parallel, angles 1e-15 .. 1e-4"] = (np.c_[p, p + d * l1], np.c_[p + o + d * sh, p + o + d * sh + d2 * l2])
    # degenerate around EPS = 1e-18 (squared length): lengths 1e-11 .. 1e-7 and exactly zero, one segment or both
    p1, p2 = rp(m), rp(m)
    ln = np.where(rng.random((m, 1)) < 0.25, 0.0, 10.0 ** rng.uniform(-11, -7, (m, 1)))
    ln2 = np.where(rng.random((m, 1)) < 0.25, 0.0, 10.0 ** rng.uniform(-11, -7, (m, 1)))
    both = (np.arange(m) % 3 == 0)[:, None]
    e1 = unit(rng.normal(size=(m, 3))) * ln
    e2 = unit(rng.normal(size=(m, 3))) * np.where(both, ln2, rng.uniform(0.05, 1.0, (m, 1)))
    close = (np.arange(m) % 2 == 0)[:, None]  # half of them near the other segment, where a wrong branch shows
    p1 = np.where(close, p2 + e2 * rng.uniform(-0.5, 1.5, (m, 1)) + unit(rng.normal(size=(m, 3))) * 10.0 ** rng.uniform(-9, -3, (m, 1)), p1)
    swap = (np.arange(m) % 4 < 2)[:, None]
    a, b = np.c_[p1, p1 + e1], np.c_[p2, p2 + e2]
    fam["degenerate around EPS"] = (np.where(swap, a, b), np.where(swap, b, a))
    # every clamp combination: s and t each below 0, inside, above 1 -- built from the closest points of the two LINES
    segs_a, segs_b = [], []
    for cs in (-1, 0, 1):
        for ct in (-1, 0, 1):
            k = 40
            c, d1, d2 = rp(k), unit(rng.normal(size=(k, 3))), unit(rng.normal(size=(k, 3)))
            gap = unit(np.cross(d1, d2)) * rng.uniform(0.0, 0.2, (k, 1))
            span = lambda c_: {-1: (0.1, 0.6), 0: (-0.3, 0.3), 1: (-0.6, -0.1)}[c_]  # where the segment lies relative to the lines' closest point
            (a0, a1), (b0, b1) = span(cs), span(ct)
            segs_a.append(np.c_[c + d1 * a0, c + d1 * a1])
            segs_b.append(np.c_[c + gap + d2 * b0, c + gap + d2 * b1])
    fam["every clamp combination of s and t"] = (np.vstack(segs_a), np.vstack(segs_b))
    return fam


def test_segseg_distance_is_a_lower_bound(lib):
    fams = seg_seg_families(np.random.default_rng(32))
    total = 0
    print()
    for name, (a, b) in fams.items():
        got = np.sqrt(vc.segseg_dist2(lib, a, b))
        br = np.array([sc.core_bracket(_points_core(s), _points_core(t)) for s, t in zip(a, b)])
        ok = (br[:, 1] - br[:, 0]) <= 1e-9  # (as above: every case is held to up; the shortfall below lo is quoted on the narrow brackets)
        excess, below = got - br[:, 1], (br[:, 0] - got)[ok]
        total += len(a)
        print(f"  seg<->seg {name:38s} {len(a):4d} cases ({int(ok.sum())} brackets within 1e-9), bound - up: largest {excess.max():+.2e}; "
              f"below lo by at most {below.max():+.2e} (not asserted)")
        assert excess.max() <= sc.LD_TOL, (name, "segseg_dist2 overstates the distance by", excess.max(), a[np.argmax(excess)], b[np.argmax(excess)])
    assert total >= 2000


# ------------------------------------------------------------------------------------------------ c: no culled pair is in contact
def test_no_culled_pair_is_in_contact(lib, fx):
    rng = np.random.default_rng(33)
    rand = np.c_[rng.uniform(-np.pi, np.pi, 2000), rng.uniform(-np.pi, 0.0, 2000), rng.uniform(-np.pi, np.pi, (2000, 4))]
    q = np.vstack([fx["q"], rand])
    print()
    for margin in (0.01, 0.0, 0.05):
        root, squared, bound = vc.cull_masks(lib, q, margin)
        assert ((root & ~squared) == 0).all()  # (the squared form keeps what the root form keeps: tests/test_p1_cull_host.py)
        culled = checked = 0
        tightest = np.inf
        for e in range(len(q)):
            bits = [i for i in range(19) if not (root[e] >> i) & 1]
            culled += len(bits)
            near = [vc.N_OBST + i for i in bits if bound[e, i] - margin <= 0.02]
            if not near:
                continue
            lo, _ = vc.pair_brackets(q[e], None, decide=margin, only=near)
            checked += len(near)
            tightest = min(tightest, (lo[near] - margin).min())
            assert (lo[near] > margin).all(), ("a culled pair is in contact", margin, e, q[e], [(vc.PAIR_NAMES[k], lo[k]) for k in near if lo[k] <= margin])
        print(f"  margin {margin}: {len(q)} poses, {culled} culled pairs, {checked} with the capsule bound within 2 cm of the reach, all certified lo > margin "
              f"(closest: certified lower bound {tightest:+.3e} above the margin)")
        assert checked >= 100


# ------------------------------------------------------------------------------------------------ d: the fixture says what it claims
def test_fixture_sample_is_recertified(fx):
    n = len(fx["pair"])
    pick = np.random.default_rng(34).choice(n, 60, replace=False)
    worst = [0.0, 0.0, np.inf]
    for i in pick:
        p = int(fx["pair"][i])
        lo, up = vc.pair_brackets(fx["q"][i], fx["obst"][i], only=(p,))
        assert abs(lo[p] - fx["lo"][i]) <= 1e-13 and abs(up[p] - fx["up"][i]) <= 1e-13, (i, "the committed bracket is not reproduced")
        assert up[p] - lo[p] <= vc.BRACKET_CAP and abs(up[p] - (M + fx["gap"][i])) <= vc.GAP_TOL, (i, vc.PAIR_NAMES[p], fx["gap"][i], lo[p], up[p])
        others = [k for k in range(vc.N_PAIRS) if k != p]
        olo, _ = vc.pair_brackets(fx["q"][i], fx["obst"][i], decide=M + vc.ISOLATION, only=others)
        assert (olo[others] > M + vc.ISOLATION).all(), (i, "another pair is not certified free", [(vc.PAIR_NAMES[k], olo[k]) for k in others if olo[k] <= M + vc.ISOLATION])
        worst = [max(worst[0], up[p] - lo[p]), max(worst[1], abs(up[p] - (M + fx["gap"][i]))), min(worst[2], olo[others].min() - M)]
    print(f"\n  60 of {n} poses re-certified: widest bracket {worst[0]:.1e}, gap held to {worst[1]:.1e}, others at least {worst[2]:.2e} above the margin")
    assert (fx["others_lo"] > M + vc.ISOLATION).all() and (fx["up"] - fx["lo"] <= vc.BRACKET_CAP).all()
    assert (np.abs(fx["up"] - (M + fx["gap"])) <= vc.GAP_TOL).all()


@pytest.mark.parametrize("has_obstacle", [False, True])
def test_oracle_verdict_obeys_the_rule(oracle, fx, has_obstacle):
    n = len(fx["pair"])
    got = np.array([oracle.query(fx["q"][i], fx["obst"][i] if has_obstacle else None)[1] for i in range(n)])
    table = vc.assert_verdicts(oracle, got, got, fx, np.arange(n), has_obstacle, "oracle")
    exp = vc.expected(fx, has_obstacle)
    print("\n" + "\n".join(vc.table_lines(table, f"oracle, {'with' if has_obstacle else 'without'} the obstacle")))
    print(f"  {n} poses: {int((exp == 'free').sum())} certainly free, {int((exp == 'colliding').sum())} certainly colliding, {int((exp == 'band').sum())} in the band "
          f"(oracle: {int(got[exp == 'band'].sum())} of them colliding)")


# ------------------------------------------------------------------------------------------------ e: coverage
def test_fixture_coverage(fx):
    assert len(vc.UNREACHED) <= 4 and set(vc.UNREACHED) <= set(vc.PAIR_NAMES)
    directed = fx["family"] == vc.FAMILY_DIRECTED
    for p, name in enumerate(vc.PAIR_NAMES):
        for g in vc.GAPS:
            count = int((directed & (fx["pair"] == p) & (fx["gap"] == g)).sum())
            if name in vc.UNREACHED:
                assert count == 0, (name, "is listed as unreached and has poses")
            else:
                assert count >= vc.POSES_PER_CELL, (name, g, count)
    assert sum(g < 0 for g in vc.GAPS) >= 6 and sum(g > 0 for g in vc.GAPS) >= 4
    tight = fx["family"] == vc.FAMILY_TIGHT
    assert tight.sum() == vc.TIGHT_COUNT
    assert set(fx["pair"][tight]) <= set(range(vc.N_OBST, vc.N_OBST + 10)) and set(np.abs(fx["gap"][tight])) <= {abs(g) for g in vc.TIGHT_GAPS}
    exp = vc.expected(fx, True)
    assert {"free", "colliding", "band"} == set(exp)
