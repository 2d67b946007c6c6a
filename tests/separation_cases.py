"""Query sets and the independent reference of the separation-distance tests (tests/test_separation_host.py on the CPU,
tests/test_separation.py on the GPU).  Everything here is host numpy; nothing touches the device, and nothing is shared with the
Voronoi simplex of the oracle or of urgym_device.h.

A query is the 6-tuple of oracle.closest / env.probe_closest: (type_a, par_a, pose_a, type_b, par_b, pose_b), pose = xyz + quaternion
xyzw.  Cores and margins are those penetration_cases.py states: a hull is the vertex set of data/ur5e_model.npz with margin 1 mm, a box
has core half extents - 1 mm, a cylinder core radius - 1 mm and core half height - 1 mm about z (margin 1 mm each), a sphere is a
point whose margin is its radius.

THE CERTIFICATE.  Let D = core_A - core_B (a convex set) and d* = min |x| over x in D, the core distance.
  * every point v of D has |v| >= d*: an UPPER bound;
  * for every direction v != 0, with w = the point of D that minimises v.x (the support point of D in direction -v),
    every x in D has v.x >= v.w, hence |x| >= v.w / |v|: a LOWER bound.
exact_separation keeps the best of each over a search; (lo, up) = that pair minus both margins brackets the distance p.getClosestPoints
reports.  HOW the points v are found cannot make the bracket wrong, only wide, and a wide bracket (> BRACKET_CAP) is dropped and
counted, never trusted.
"""
import itertools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = np.load(os.path.join(ROOT, "data", "ur5e_model.npz"))
FIXTURE = os.path.join(ROOT, "tests", "golden", "separation_queries.npz")
HULL, CYLZ, BOX, SPHERE = 0, 1, 2, 3
MARGIN = 0.001                      # hull, box, cylinder
CYL = [0.05, 0.4, 0.0]              # the obstacle: radius, height
TABLE_HALF, TRACK_HALF, CUBE_HALF = [0.55, 0.9, 0.46], [0.1, 0.55, 0.06], [0.025, 0.025, 0.025]
TABLE_POSE, TRACK_POSE = np.r_[0.5, 0.0, -0.58, 0, 0, 0, 1.0], np.r_[0.0, 0.0, -0.06, 0, 0, 0, 1.0]
SPHERE_R = 0.02

STOP, MAX_ITER = 1.0e-14, 300       # the search ends at up - lo <= STOP or after MAX_ITER support calls
STALL = 4                           # ... or after this many calls in a row that improved neither bound (the rounding floor)
BRACKET_CAP = 1.0e-12               # a wider bracket is dropped and counted
DROP_SHARE = 0.01                   # ... and no family may lose more than this share
BELOW_TOL = 1.0e-12                 # d >= lo - BELOW_TOL: |v| of a search is the norm of a point of A - B, only rounding is below d*
LD_TOL = 1.0e-8                     # the project's link-distance tolerance (tests/test_gpu_parity.py): d <= up + LD_TOL on the stable set
# Off the stable set (sliver exit: the previous v stands, unconverged) d - up <= SLIVER_CAP = twice the largest excess of the ORACLE
# over the reference on the committed query sets, measured on the CPU by tests/golden/gen_separation_queries.py (which prints it;
# DESIGN.md section 3 records the run): the factor two because a kernel may legitimately land on another of the oracle's branches.
ORACLE_MAX_EXCESS = 1.3085e-04
SLIVER_CAP = 2.0 * ORACLE_MAX_EXCESS
PERTURB, PERTURB_RUNS, STABLE_SPAN = 1.0e-14, 50, 1.0e-12  # the stable set: 50 moves of A by 1e-14, no exit 3, answers within 1e-12
SLIVER_EXIT = 3


# ------------------------------------------------------------------------------------------------ shapes
def quat_to_matrix(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def matrix_to_quat(R):
    """xyzw of a rotation matrix (Shepperd's branches)."""
    t = np.trace(R)
    c = [R[0, 0], R[1, 1], R[2, 2], t]
    k = int(np.argmax(c))
    if k == 3:
        q = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], 1.0 + t])
    else:
        i, j, l = k, (k + 1) % 3, (k + 2) % 3
        q = np.zeros(4)
        q[i] = 1.0 + R[i, i] - R[j, j] - R[l, l]
        q[j] = R[i, j] + R[j, i]
        q[l] = R[i, l] + R[l, i]
        q[3] = R[l, j] - R[j, l]
    return q / np.linalg.norm(q)


_HULLS = np.split(MODEL["hull_verts"], MODEL["hull_offset"][1:-1])
_JOINT_XYZ, _JOINT_RPY = MODEL["joint_xyz"], MODEL["joint_rpy"]


def hull_verts(link):
    return _HULLS[link - 1]


_CORNERS = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)


class Core:
    """A core shape in the world frame: a vertex set (hull, box, sphere centre) or a cylinder; support(d) maximises d.x."""

    def __init__(self, typ, par, pose=None, frame=None):
        """pose = xyz + quaternion xyzw, or frame = (R, t)."""
        if frame is None:
            pose = np.asarray(pose, np.float64)
            frame = quat_to_matrix(pose[3:]), pose[:3].copy()
        self.R, self.t = frame
        self.cyl = None
        if typ == HULL:
            local, self.margin = hull_verts(int(par[0])), MARGIN
        elif typ == BOX:
            local, self.margin = _CORNERS * (np.asarray(par[:3], np.float64) - MARGIN), MARGIN
        elif typ == SPHERE:
            local, self.margin = np.zeros((1, 3)), float(par[0])
        else:
            assert typ == CYLZ
            local, self.margin = None, MARGIN
            self.cyl = (float(par[0]) - MARGIN, 0.5 * float(par[1]) - MARGIN)
        self.verts = None if local is None else local @ self.R.T + self.t

    def support(self, d):
        if self.verts is not None:
            return self.verts[int(np.argmax(self.verts @ d))]
        r, h = self.cyl
        l = self.R.T @ d
        s = np.hypot(l[0], l[1])
        p = np.array([r * l[0] / s, r * l[1] / s, h if l[2] >= 0 else -h]) if s > 0 else np.array([r, 0.0, h if l[2] >= 0 else -h])
        return self.R @ p + self.t


# ------------------------------------------------------------------------------------------------ the reference
_SUBSETS = {k: [list(c) for m in range(1, k + 1) for c in itertools.combinations(range(k), m)] for k in range(1, 5)}


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _affine_coordinates(S):
    """Barycentric coordinates of the point of the affine hull of S (2, 3 or 4 points, lists of floats) closest to the origin, in
    closed form on the edge vectors themselves (no Gram matrix: its condition number would be the square); None for a flat S."""
    s0 = S[0]
    E = [[p[0] - s0[0], p[1] - s0[1], p[2] - s0[2]] for p in S[1:]]
    m = [-s0[0], -s0[1], -s0[2]]
    if len(E) == 1:
        den = _dot(E[0], E[0])
        mu = None if den == 0.0 else [_dot(m, E[0]) / den]
    elif len(E) == 2:
        n = _cross(E[0], E[1])  # the plane's normal: the component of m along it drops out of both triple products
        den = _dot(n, n)
        mu = None if den == 0.0 else [_dot(_cross(m, E[1]), n) / den, _dot(_cross(E[0], m), n) / den]
    else:
        c12, c20, c01 = _cross(E[1], E[2]), _cross(E[2], E[0]), _cross(E[0], E[1])
        den = _dot(E[0], c12)
        mu = None if den == 0.0 else [_dot(m, c12) / den, _dot(m, c20) / den, _dot(m, c01) / den]
    return None if mu is None else [1.0 - sum(mu)] + mu


def _affine_coordinates_lstsq(S):
    """The same by least squares (SVD) on the edge matrix: slower, and the fallback where the closed form's rounding stalls a search."""
    S = np.array(S)
    mu = np.linalg.lstsq((S[1:] - S[0]).T, -S[0], rcond=None)[0]
    return [1.0 - float(mu.sum())] + mu.tolist()


def closest_in_hull(P, coordinates=_affine_coordinates):
    """The point of conv(P) closest to the origin, P of at most four points, by brute force: for every non-empty subset the
    point of its AFFINE hull closest to the origin, kept when all its barycentric coordinates are non-negative -- then it is a
    point of conv(P), whatever the conditioning of the solve; the true closest point lies in the relative interior of some face and
    is that face's candidate, so the shortest kept candidate is it.  Returns (point, the rows of P that carry it)."""
    pts = P.tolist()
    best, best_n2, best_rows = None, np.inf, None
    for rows in _SUBSETS[len(pts)]:
        S = [pts[r] for r in rows]
        lam = [1.0] if len(rows) == 1 else coordinates(S)
        if lam is None or min(lam) < 0.0:
            continue  # (a flat subset's hull is covered by its own subsets)
        x = [sum(l * p[k] for l, p in zip(lam, S)) for k in range(3)]
        n2 = _dot(x, x)
        if n2 < best_n2:
            best, best_n2, best_rows = x, n2, [r for r, l in zip(rows, lam) if l > 0.0]
    return np.array(best), best_rows


def core_bracket(A, B, decide=None):
    """(lo, up) of the distance between the cores A and B (module docstring); (0, 0) when the search reaches the origin.
    decide: the search may also end as soon as the bracket excludes this value (all a bisection asks of it)."""
    sup = lambda d: A.support(d) - B.support(-d)
    v = sup(B.t - A.t if np.any(B.t != A.t) else np.array([1.0, 0.0, 0.0]))
    P = v[None, :]
    lo, up, idle, coordinates = 0.0, np.inf, 0, _affine_coordinates
    for _ in range(MAX_ITER):
        nv = np.sqrt(v @ v)
        if nv == 0.0:
            up = 0.0
            break
        w = sup(-v)
        low = (v @ w) / nv
        idle = 0 if (nv < up or low > lo) else idle + 1
        lo, up = max(lo, low), min(up, nv)
        if up - lo <= STOP or (decide is not None and not lo <= decide <= up):
            break
        if idle >= STALL or (np.abs(P - w).max(1) == 0.0).any():
            # no bound moves any more, or the support point is in the set already: the rounding floor of the closed-form solve.  Once,
            # the search goes on with the least-squares solve; the second time it ends.
            if coordinates is _affine_coordinates_lstsq:
                break
            coordinates, idle = _affine_coordinates_lstsq, 0
            if (np.abs(P - w).max(1) == 0.0).any():
                v, rows = closest_in_hull(P, coordinates)
                P = P[rows]
                continue
        cand = np.vstack([P, w])  # at most three kept points and the new one
        v, rows = closest_in_hull(cand, coordinates)
        P = cand[rows]
        if len(P) == 4:  # the origin is inside a tetrahedron of D (only rounding keeps |v| off zero): drop the oldest point
            P = P[1:]
    return lo, up


def exact_separation(query, decide=None):
    """(lo, up): certified bounds of the distance between the margin-inflated shapes of the query, lo <= truth <= up.
    decide: see core_bracket (a distance between the inflated shapes)."""
    ta, pa, xa, tb, pb, xb = query
    A, B = Core(ta, pa, xa), Core(tb, pb, xb)
    m = A.margin + B.margin
    lo, up = core_bracket(A, B, None if decide is None else decide + m)
    return lo - m, up - m


# ------------------------------------------------------------------------------------------------ forward kinematics
def _rpy_matrix(rpy):
    """URDF's fixed-axis roll-pitch-yaw: R = Rz(yaw) Ry(pitch) Rx(roll)."""
    (cr, cp, cy), (sr, sp, sy) = np.cos(rpy), np.sin(rpy)
    rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return rz @ ry @ rx


def numpy_fk(q):
    """World frames of links 0..6 from joint_xyz / joint_rpy of the model file: (R [7, 3, 3], t [7, 3]).  Written from the URDF's
    joint origins, not from the oracle's table of joint rotations."""
    R, t = np.eye(3), np.zeros(3)
    Rs, ts = [R], [t]
    for k in range(6):
        c, s = np.cos(q[k]), np.sin(q[k])
        t = t + R @ _JOINT_XYZ[k]
        R = R @ _rpy_matrix(_JOINT_RPY[k]) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
        Rs.append(R)
        ts.append(t)
    return np.array(Rs), np.array(ts)


def link_brackets(q, obst_pose, workbench=False):
    """(lo [5], up [5]) of one env's link_dist cells: links 2..6 against the obstacle cylinder; under WORKBENCH the minimum of the
    three bodies' lo and of their up (the minimum of the truths lies between the two)."""
    R, t = numpy_fk(q)
    bodies = [Core(CYLZ, CYL, obst_pose)]
    if workbench:
        bodies += [Core(BOX, TABLE_HALF, TABLE_POSE), Core(BOX, TRACK_HALF, TRACK_POSE)]
    lo, up = np.zeros(5), np.zeros(5)
    for i, link in enumerate(range(2, 7)):
        A = Core(HULL, [link], frame=(R[link], t[link]))
        br = np.array([core_bracket(A, B) for B in bodies]) - 2 * MARGIN
        lo[i], up[i] = br[:, 0].min(), br[:, 1].min()
    return lo, up


# ------------------------------------------------------------------------------------------------ query families
FAR = ("far hull<->cyl", "far hull<->table", "far hull<->track", "far hull<->hull", "far sphere<->cyl", "far cube<->cyl", "far hull<->cube")
NEAR = {"near hull<->cyl": 250, "near sphere<->cyl": 250, "near hull<->cube": 100, "near hull<->hull": 100}
FAMILIES = FAR + tuple(NEAR)
FAR_COUNT, GAP_LO, GAP_HI = 150, 1.0e-4, 2.0e-2


def _rand_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def _shapes(fam, rng):
    a, b = fam.split(" ")[1].split("<->")
    one = lambda s, lo: (HULL, [int(rng.integers(lo, 7)), 0, 0]) if s == "hull" else {
        "cyl": (CYLZ, CYL), "table": (BOX, TABLE_HALF), "track": (BOX, TRACK_HALF), "cube": (BOX, CUBE_HALF), "sphere": (SPHERE, [SPHERE_R, 0, 0])}[s]
    return one(a, 1), one(b, 1)


def far_queries(fam, seed):
    """Poses drawn as in test_device_gjk_matches_oracle_on_host: A in [-0.4, 0.4]^2 x [0, 0.8], B in [-0.6, 0.6]^2 x [-0.6, 0.9],
    both rotated at random -- except the table and the track, which stand where the scene has them (a table posed at random in
    that box overlaps every second hull, and the census allows 10 % of a family to be penetrating and skipped)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(FAR_COUNT):
        (ta, pa), (tb, pb) = _shapes(fam, rng)
        xa = np.r_[rng.uniform([-0.4, -0.4, 0.0], [0.4, 0.4, 0.8]), _rand_quat(rng)]
        xb = np.r_[rng.uniform([-0.6, -0.6, -0.6], [0.6, 0.6, 0.9]), _rand_quat(rng)]
        xb = {"table": TABLE_POSE, "track": TRACK_POSE}.get(fam.split("<->")[1], xb)
        out.append((ta, pa, xa, tb, pb, xb))
    return out


def slide_to_gap(ta, pa, qa, tb, pb, xb, direction, gap, anchor=None, reach=3.0):
    """A (orientation qa) slides along `direction` through `anchor` (B's centre by default, taken by A's own centre: its hull's
    centroid) until the REFERENCE's distance equals `gap`: bisection on exact_separation's upper bound between the anchor (cores
    overlap or nearly) and `reach` metres out.  Returns A's pose."""
    Ra = quat_to_matrix(qa)
    centre = Ra @ hull_verts(int(pa[0])).mean(0) if ta == HULL else np.zeros(3)
    anchor = np.asarray(xb[:3], np.float64) if anchor is None else anchor
    pose = lambda s: np.r_[anchor + s * direction - centre, qa]
    f = lambda s: exact_separation((ta, pa, pose(s), tb, pb, xb), decide=gap)[1] - gap
    s0, s1 = 0.0, reach
    assert f(s1) > 0.0
    if f(s0) > 0.0:
        return None  # (the line misses B by more than the gap at the anchor: the caller draws again)
    for _ in range(60):
        mid = 0.5 * (s0 + s1)
        if f(mid) > 0.0:
            s1 = mid
        else:
            s0 = mid
        if s1 - s0 < 1e-15:
            break
    return pose(s1)


def near_queries(fam, seed):
    """B posed at random; A slides along a random line through B's centre until the reference's distance is a gap drawn log-uniformly
    from 1e-4 .. 2e-2 m: around the 0.01 m collision margin, where the simplices are small."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < NEAR[fam]:
        (ta, pa), (tb, pb) = _shapes(fam, rng)
        xb = np.r_[rng.uniform([-0.6, -0.6, -0.6], [0.6, 0.6, 0.9]), _rand_quat(rng)]
        d = rng.normal(size=3)
        gap = float(np.exp(rng.uniform(np.log(GAP_LO), np.log(GAP_HI))))
        anchor = xb[:3] if tb != HULL else xb[:3] + quat_to_matrix(xb[3:]) @ hull_verts(int(pb[0])).mean(0)
        xa = slide_to_gap(ta, pa, _rand_quat(rng), tb, pb, xb, d / np.linalg.norm(d), gap, anchor=anchor)
        if xa is not None:
            out.append((ta, pa, xa, tb, pb, xb))
    return out


# Fixed seeds.  Against the cylinder few near-contact searches end cleanly (3.6 % of hull, 5.7 % of sphere queries over the seeds
# 100 .. 111), so 250 queries hold 5 .. 17 stable ones depending on the draw, and the census asks for 10: the two
# cylinder families take the seed of 100 .. 111 with the most.  That choice is made on the oracle's side alone.
SEEDS = {fam: 100 + k for k, fam in enumerate(FAMILIES)}
SEEDS.update({"near hull<->cyl": 101, "near sphere<->cyl": 101})


def generate_queries():
    """All families with their fixed seeds: a list of (family, query)."""
    out = []
    for fam in FAMILIES:
        out += [(fam, q) for q in (far_queries(fam, SEEDS[fam]) if fam in FAR else near_queries(fam, SEEDS[fam]))]
    return out


def save_fixture(path, cases, brackets):
    q = [c[1] for c in cases]
    par = lambda k: np.array([np.r_[np.asarray(x[k], np.float64), np.zeros(3)][:3] for x in q])
    np.savez_compressed(path, family=np.array([FAMILIES.index(c[0]) for c in cases], np.int8), families=np.array(FAMILIES),
                        type_a=np.array([x[0] for x in q], np.int8), type_b=np.array([x[3] for x in q], np.int8), par_a=par(1), par_b=par(4),
                        pose_a=np.array([x[2] for x in q]), pose_b=np.array([x[5] for x in q]), lo=brackets[:, 0], up=brackets[:, 1])


def load_fixture(path=FIXTURE):
    """(cases, lo, up): cases = [(family, query)] as generate_queries() made them, with the reference's bracket of each."""
    z = np.load(path)
    assert tuple(z["families"]) == FAMILIES
    cases = [(FAMILIES[f], (int(ta), list(pa), xa, int(tb), list(pb), xb))
             for f, ta, pa, xa, tb, pb, xb in zip(z["family"], z["type_a"], z["par_a"], z["pose_a"], z["type_b"], z["par_b"], z["pose_b"])]
    return cases, z["lo"], z["up"]


# ------------------------------------------------------------------------------------------------ the oracle's side
def oracle_rows(oracle, cases, seed=0):
    """For every (family, query): the oracle's distance, penetrating flag and exit code, and whether the query is in the STABLE
    set -- under PERTURB_RUNS moves of A's position by PERTURB the oracle never takes the sliver exit and its answers span at most
    STABLE_SPAN -- with the range [d_min, d_max] of those answers (the unperturbed one included)."""
    rng = np.random.default_rng(seed)
    rows = []
    for fam, q in cases:
        r = oracle.closest(*q)
        row = dict(family=fam, distance=r["distance"], penetrating=r["penetrating"], exit=oracle.last_gjk_exit())
        vals, sliver = [r["distance"]], row["exit"] == SLIVER_EXIT
        if not r["penetrating"]:
            for _ in range(PERTURB_RUNS):
                p = oracle.closest(q[0], q[1], np.r_[q[2][:3] + rng.normal(0, PERTURB, 3), q[2][3:]], q[3], q[4], q[5])
                vals.append(p["distance"])
                sliver |= oracle.last_gjk_exit() == SLIVER_EXIT or p["penetrating"]
        row.update(d_min=min(vals), d_max=max(vals), stable=not r["penetrating"] and not sliver and max(vals) - min(vals) <= STABLE_SPAN)
        rows.append(row)
    return rows


def kept(lo, up):
    """The queries whose bracket is narrow enough to judge by."""
    return (up - lo) <= BRACKET_CAP


def census_table(rows, lo, up, values=None, title="oracle"):
    """Text lines by family and exit of the ORACLE's search: count, share of the family's separated queries and the largest excess
    of `values` (the oracle's own distances by default) over the reference's upper bound."""
    d = np.array([r["distance"] for r in rows]) if values is None else np.asarray(values)
    lines = [f"  {title}: family, separated / queries (stable), then per oracle exit: count, share, largest d - up"]
    for fam in FAMILIES:
        idx = [k for k, r in enumerate(rows) if r["family"] == fam]
        sep = [k for k in idx if not rows[k]["penetrating"] and kept(lo[k], up[k])]
        cells = []
        for ex in sorted({rows[k]["exit"] for k in sep}):
            ks = [k for k in sep if rows[k]["exit"] == ex]
            cells.append(f"exit {ex}: {len(ks)} ({100.0 * len(ks) / len(sep):.0f} %) {max(d[k] - up[k] for k in ks):+.2e}")
        lines.append(f"  {fam:18s} {len(sep):3d} / {len(idx):3d} ({sum(rows[k]['stable'] for k in sep):3d} stable)  " + "; ".join(cells))
    return lines


def assert_census_conditions(rows, lo, up):
    """What the comparison must cover, stated on the oracle's and the reference's side only."""
    for fam in FAMILIES:
        idx = [k for k, r in enumerate(rows) if r["family"] == fam]
        dropped = sum(not kept(lo[k], up[k]) for k in idx)
        assert dropped <= DROP_SHARE * len(idx), (fam, "dropped", dropped)
        stable = sum(rows[k]["stable"] and kept(lo[k], up[k]) for k in idx)
        if fam in FAR:
            assert sum(rows[k]["penetrating"] for k in idx) <= 0.10 * len(idx), (fam, "penetrating and skipped")
            assert stable >= 30, (fam, "stable", stable)
        else:
            assert stable >= 10, (fam, "stable", stable)
    assert sum(r["exit"] == SLIVER_EXIT and not r["penetrating"] for r in rows) >= 100, "sliver exits"


def assert_against_bracket(d, rows, lo, up, what):
    """The three bounds on every separated query with a kept bracket; returns the largest excess on and off the stable set."""
    worst = [0.0, 0.0]
    for k, r in enumerate(rows):
        if r["penetrating"] or not kept(lo[k], up[k]):
            continue
        assert d[k] >= lo[k] - BELOW_TOL, (what, "below the truth", k, r["family"], d[k], lo[k])
        bound = LD_TOL if r["stable"] else SLIVER_CAP
        assert d[k] - up[k] <= bound, (what, "stable" if r["stable"] else "sliver", k, r["family"], r["exit"], d[k], up[k])
        worst[not r["stable"]] = max(worst[not r["stable"]], d[k] - up[k])
    return worst


def assert_cells_against_brackets(state, workbench, what):
    """The link_dist cells [5, N] of a state (q, obst_pos, obst_quat, link_dist: get_state() or the oracle's buffers) against the
    brackets of link_brackets at that state's own joint angles and obstacle pose.  Every cell that is non-negative, and every cell at
    which the reference itself is positive, is held to d >= lo - BELOW_TOL and d - up <= SLIVER_CAP; the other negative cells are
    penetration depths (or margins that overlap) and are counted.  Cells whose bracket is wider than BRACKET_CAP are dropped and
    counted.  Returns dict(cells, negative, dropped, excess = the largest d - up)."""
    ld = np.asarray(state["link_dist"], np.float64)
    out = dict(cells=ld.size, negative=0, dropped=0, excess=-np.inf)
    for n in range(ld.shape[1]):
        lo, up = link_brackets(state["q"][:, n], np.concatenate((state["obst_pos"][:, n], state["obst_quat"][:, n])), workbench)
        for i in range(5):
            d = ld[i, n]
            if not kept(lo[i], up[i]):
                out["dropped"] += 1
            elif d < 0.0 and lo[i] <= 0.0:
                out["negative"] += 1
            else:
                assert d >= lo[i] - BELOW_TOL, (what, "below the truth", "link", i + 2, "env", n, d, lo[i])
                assert d - up[i] <= SLIVER_CAP, (what, "above the truth", "link", i + 2, "env", n, d, up[i])
                out["excess"] = max(out["excess"], d - up[i])
    return out


def refresh_near_state(n=48, seed=9):
    """State for set_state(..., refresh=True) / load_state + refresh: random joint angles, and in every env the obstacle placed by the
    reference (as the near families are: a slide along a random line, here of the cylinder through the centroid of link 2 + env % 5)
    so that its distance from that link is a gap drawn log-uniformly from GAP_LO .. GAP_HI.  Returns (state, links, gaps); the
    state holds q [6, n] and obst_start [6, n] as xyz + rpy with yaw 0 (the cylinder is symmetric about its axis)."""
    rng = np.random.default_rng(seed)
    q = np.c_[rng.uniform(-np.pi, np.pi, n), rng.uniform(-2.2, -0.4, n), rng.uniform(-2, 2, (n, 4))]
    obst, links, gaps = np.zeros((n, 6)), 2 + np.arange(n) % 5, np.exp(rng.uniform(np.log(GAP_LO), np.log(GAP_HI), n))
    for e in range(n):
        R, t = numpy_fk(q[e])
        A = Core(HULL, [links[e]], frame=(R[links[e]], t[links[e]]))
        while True:
            rpy = np.r_[rng.uniform(-2.6, 2.6, 2), 0.0]
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            Rb, anchor = _rpy_matrix(rpy), A.verts.mean(0)
            f = lambda s: core_bracket(A, Core(CYLZ, CYL, frame=(Rb, anchor + s * d)), decide=gaps[e] + 2 * MARGIN)[1] - 2 * MARGIN - gaps[e]
            if f(0.0) < 0.0:
                break
        s0, s1 = 0.0, 2.0
        for _ in range(32):  # (to 5e-10 m: the gap is drawn, not prescribed to the last digit)
            mid = 0.5 * (s0 + s1)
            s0, s1 = (s0, mid) if f(mid) > 0.0 else (mid, s1)
        obst[e] = np.r_[anchor + s1 * d, rpy]
    return {"q": q.T.copy(), "obst_start": obst.T.copy()}, links, gaps


def assert_refresh_coverage(state, links, gaps):
    """On the reference's side: in the state a refresh left, the targeted link of every env is GAP_LO .. GAP_HI from the obstacle, at
    the gap refresh_near_state asked for (to 1e-8: its bisection stops at 5e-10, and the angles of obst_start go through the project's own
    conversion)."""
    for e, (link, gap) in enumerate(zip(links, gaps)):
        lo, up = link_brackets(state["q"][:, e], np.concatenate((state["obst_pos"][:, e], state["obst_quat"][:, e])))
        assert GAP_LO - 1e-9 <= lo[link - 2] and up[link - 2] <= GAP_HI + 1e-9 and abs(up[link - 2] - gap) <= 1e-8, (e, link, gap, lo, up)
