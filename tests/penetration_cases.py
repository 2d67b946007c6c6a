"""Query sets and the independent reference of the penetration-depth tests (tests/test_penetration_depth.py on the GPU, the
oracle-only halves in tests/test_oracle.py).  Everything here is host numpy + the CPU oracle; nothing touches the device.

A query is the 6-tuple of oracle.closest / env.probe_closest: (type_a, par_a, pose_a, type_b, par_b, pose_b), pose = xyz + quaternion
xyzw.  The margins (0.001 for hulls, boxes and cylinders, the radius for a sphere) are those of oracle/urgym_oracle.cpp.
"""
import os

import numpy as np
from scipy.spatial import ConvexHull
from scipy.spatial.transform import Rotation as Rot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = np.load(os.path.join(ROOT, "data", "ur5e_model.npz"))
HULL, CYLZ, BOX, SPHERE = 0, 1, 2, 3
IDENT = [0.0, 0.0, 0.0, 1.0]
MARGIN = 0.001                      # hull, box, cylinder
EPA_TOL, EPA_CAP = 1.0e-9, 44       # the project's constants: convergence of the search, expansions at the 48-point cap
TABLE = (BOX, [0.55, 0.9, 0.46], np.r_[0.5, 0.0, -0.58, IDENT])
TRACK = (BOX, [0.1, 0.55, 0.06], np.r_[0.0, 0.0, -0.06, IDENT])
CUBE_HALF = [0.025, 0.025, 0.025]   # the 2.5 cm cube (the target box of UR5StaReach-v1)
CYL = [0.05, 0.4, 0.0]              # the obstacle: radius, height


def hull_verts(link):
    o = MODEL["hull_offset"]
    return MODEL["hull_verts"][o[link - 1]:o[link]]


def rand_quat(rng):
    return Rot.random(random_state=int(rng.integers(1 << 30))).as_quat()


# ------------------------------------------------------------------------------------------------ exact reference (polytopes)
# depth(cores) = min over unit n of h_{A-B}(n).  For two convex polytopes the minimum is attained at a facet normal of the
# Minkowski difference A - B, and every facet of A - B is a face of A plus a vertex of B, a vertex of A plus a face of -B, or
# an edge of A plus an edge of B: its normal is a face normal of A, minus a face normal of B, or +-(edge of A x edge of B).
# h >= depth in EVERY direction, so surplus candidates (both signs of the face normals, the diagonals qhull leaves in flat
# facets) cannot lower the minimum.  An edge pair spans a facet only if its normal n lies on the arc of outward normals of A's
# edge (between the normals n1, n2 of the two faces that meet there) and -n on that of B's edge; a point of the arc is within
# angle(n1, n2) of both ends, and pairs that fail this NECESSARY condition (with 1e-6 of slack on the cosine) are skipped --
# that is what makes hull <-> hull affordable.  Nothing here is shared with the expanding polytope of the oracle or the device:
# no search, no convergence tolerance, one matrix product over a finite candidate set.
_POLY = {}
ARC_SLACK = 1e-6


def _polytope(key, verts):
    """(verts, unit face normals, edges) in the shape's own frame; edges = (unit direction, the outward normals n1, n2 of the two
    faces that share it, n1.n2), one row per edge of qhull's triangulation."""
    if key not in _POLY:
        verts = np.asarray(verts, np.float64)
        hull = ConvexHull(verts)
        normals = hull.equations[:, :3]
        seen, ed, f1, f2 = set(), [], [], []
        for i, (tri, nb) in enumerate(zip(hull.simplices, hull.neighbors)):
            for k in range(3):  # neighbors[i][k] is the facet opposite vertex k: it shares the edge of the other two vertices
                u, v = sorted((int(tri[(k + 1) % 3]), int(tri[(k + 2) % 3])))
                if (u, v) not in seen:
                    seen.add((u, v))
                    ed.append(verts[v] - verts[u])
                    f1.append(i)
                    f2.append(int(nb[k]))
        ed = np.array(ed)
        ed /= np.linalg.norm(ed, axis=1, keepdims=True)
        n1, n2 = normals[f1], normals[f2]
        assert len(ed) == 3 * len(hull.simplices) // 2
        _POLY[key] = (verts, np.unique(np.round(normals, 14), axis=0), (ed, n1, n2, np.einsum("ij,ij->i", n1, n2)))
    return _POLY[key]


def core_polytope(typ, par):
    if typ == HULL:
        return _polytope(("hull", int(par[0])), hull_verts(int(par[0])))
    assert typ == BOX
    half = np.asarray(par[:3], np.float64) - MARGIN
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * half
    return _polytope(("box",) + tuple(half), corners)


def exact_polytope_distance(query, prune=True, chunk=4096):
    """The contact distance p.getClosestPoints reports for two OVERLAPPING polytopes: -(depth(cores) + margin_A + margin_B).
    prune=False evaluates every edge pair (the check of the pruning itself)."""
    ta, pa, xa, tb, pb, xb = query
    va, na, (ea, a1, a2, ca) = core_polytope(ta, pa)
    vb, nb, (eb, b1, b2, cb) = core_polytope(tb, pb)
    ra, rb = Rot.from_quat(xa[3:]), Rot.from_quat(xb[3:])
    wa, wb = ra.apply(va) + xa[:3], rb.apply(vb) + xb[:3]
    ea, a1, a2, eb, b1, b2 = ra.apply(ea), ra.apply(a1), ra.apply(a2), rb.apply(eb), rb.apply(b1), rb.apply(b2)
    na, nb = ra.apply(na), rb.apply(nb)
    cand = [na, -na, nb, -nb]
    for e0 in range(0, len(ea), 64):  # blocks of A's edges against all of B's
        sl = slice(e0, e0 + 64)
        cr = np.cross(ea[sl, None, :], eb[None, :, :])
        ln = np.linalg.norm(cr, axis=2)
        ok = ln > 1e-9  # (parallel edges span no facet)
        cr = cr / np.where(ok, ln, 1.0)[:, :, None]
        da1, da2 = np.einsum("ijk,ik->ij", cr, a1[sl]), np.einsum("ijk,ik->ij", cr, a2[sl])
        db1, db2 = np.einsum("ijk,jk->ij", cr, b1), np.einsum("ijk,jk->ij", cr, b2)
        for sgn in (1.0, -1.0):
            keep = ok
            if prune:
                lim_a, lim_b = (ca[sl] - ARC_SLACK)[:, None], (cb - ARC_SLACK)[None, :]
                keep = ok & (sgn * da1 >= lim_a) & (sgn * da2 >= lim_a) & (-sgn * db1 >= lim_b) & (-sgn * db2 >= lim_b)
            cand.append(sgn * cr[keep])
    cand = np.concatenate(cand)
    best = np.inf
    wat, wbt = np.ascontiguousarray(wa.T), np.ascontiguousarray(wb.T)
    for c0 in range(0, len(cand), chunk):
        n = cand[c0:c0 + chunk]
        best = min(best, float(((n @ wat).max(1) - (n @ wbt).min(1)).min()))  # h(n) = max_a a.n - min_b b.n
    assert best > 0.0, "the cores do not overlap"
    return -(best + 2 * MARGIN)


def _surface_point(rng, half):
    """A point on the surface of the box |x_i| <= half_i, now and then on an edge or at a corner."""
    p = rng.uniform(-1, 1, 3) * half
    k = int(rng.integers(1, 4)) if rng.uniform() < 0.4 else 1
    for ax in rng.permutation(3)[:k]:
        p[ax] = half[ax] * rng.choice([-1.0, 1.0])
    return p


def polytope_queries(seed=5):
    """Part B: about 190 overlapping polytope pairs -- hull (links 2..6) <-> track, table and the 2.5 cm cube (50 each), rotated
    box <-> box (30), hull <-> hull with the 70-vertex link 6 on one side (10)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(150):
        link = 2 + k % 5
        ra = Rot.from_quat(rand_quat(rng))
        c = ra.apply(hull_verts(link).mean(0))
        typ, par, pose = (TRACK, TABLE, (BOX, CUBE_HALF, None))[k // 50]
        if pose is None:
            pose = np.r_[rng.uniform(-0.5, 0.5, 3), rand_quat(rng)]
            centre = pose[:3] + rng.normal(0, 0.02, 3)
        else:  # the hull's centroid a few cm either side of the box's surface
            s = _surface_point(rng, np.asarray(par))
            centre = pose[:3] + s * (1.0 - rng.uniform(-0.02, 0.03) / np.abs(s).max())
        out.append(("hull<->" + ("track", "table", "cube")[k // 50], (HULL, [link, 0, 0], np.r_[centre - c, ra.as_quat()], typ, par, pose)))
    for k in range(30):
        a = (CUBE_HALF, [0.1, 0.1, 0.1], [0.05, 0.02, 0.08])[k % 3]
        if k % 2:
            typ, par, pose = (TRACK, TABLE)[(k // 2) % 2]
            s = _surface_point(rng, np.asarray(par))
            pa = np.r_[pose[:3] + s + rng.normal(0, 0.01, 3), rand_quat(rng)]
        else:
            typ, par, pose = BOX, (CUBE_HALF, [0.1, 0.1, 0.1])[(k // 2) % 2], np.r_[rng.uniform(-0.5, 0.5, 3), rand_quat(rng)]
            pa = np.r_[pose[:3] + rng.normal(0, 0.02, 3), rand_quat(rng)]
        out.append(("box<->box", (BOX, a, pa, typ, par, pose)))
    for k in range(10):
        other = 1 + k % 5
        ra, rb = Rot.from_quat(rand_quat(rng)), Rot.from_quat(rand_quat(rng))
        ta = rng.uniform(-0.5, 0.5, 3)
        tb = ta + ra.apply(hull_verts(other).mean(0)) - rb.apply(hull_verts(6).mean(0)) + rng.normal(0, 0.02, 3)
        q = (HULL, [other, 0, 0], np.r_[ta, ra.as_quat()], HULL, [6, 0, 0], np.r_[tb, rb.as_quat()])
        out.append(("hull<->hull6", q if k % 2 else (q[3], q[4], q[5], q[0], q[1], q[2])))
    return out


# ------------------------------------------------------------------------------------------------ analytic cases
def analytic_cases():
    """(name, query, expected distance, tolerance): the cases of test_oracle.py::test_penetration_depth_analytic_cases and a
    shallow ladder -- aligned boxes of half 0.1 in face contact whose CORES (half 0.099) overlap by 1e-3, 1e-5, 1e-7 m."""
    at = lambda x, y, z: np.r_[x, y, z, IDENT]
    box = [0.1, 0.1, 0.1]
    cases = [
        ("sphere in cylinder, radial", (SPHERE, [0.02, 0, 0], at(0.03, 0, 0), CYLZ, CYL, at(0, 0, 0)), -(0.02 + 0.02), 1e-8),
        ("sphere in cylinder, axial", (SPHERE, [0.02, 0, 0], at(0, 0, 0.19), CYLZ, CYL, at(0, 0, 0)), -(0.01 + 0.02), 1e-8),
        ("box <-> box, face contact", (BOX, box, at(0, 0, 0), BOX, box, at(0.15, 0.02, 0.01)), -0.05, 1e-8),
        ("cube under the table top", (BOX, [0.05] * 3, at(0.5, 0, -0.15), TABLE[0], TABLE[1], TABLE[2]), -0.08, 1e-8),
    ]
    for ov in (1e-3, 1e-5, 1e-7):
        cases.append((f"ladder, core overlap {ov:g}", (BOX, box, at(0, 0, 0), BOX, box, at(2 * 0.099 - ov, 0.02, 0.01)), -(ov + 2 * MARGIN), 1e-8))
    return cases


def rigid_motion_pair():
    """A hull <-> cylinder pose and the same pose moved rigidly (test_penetration_depth_analytic_cases): equal depths to 1e-7."""
    rng = np.random.default_rng(3)
    pa = np.r_[0.4, 0.1, 0.3, Rot.random(random_state=1).as_quat()]
    pb = np.r_[0.41, 0.12, 0.33, Rot.random(random_state=2).as_quat()]
    g = Rot.random(random_state=5)
    t = rng.uniform(-1, 1, 3)
    mv = lambda p: np.r_[g.apply(p[:3]) + t, (g * Rot.from_quat(p[3:])).as_quat()]
    return (HULL, [3, 0, 0], pa, CYLZ, CYL, pb), (HULL, [3, 0, 0], mv(pa), CYLZ, CYL, mv(pb))


# ------------------------------------------------------------------------------------------------ stratified families
FAMILIES = ("hull<->cyl shallow", "hull<->cyl deep", "sphere<->cyl", "box<->cyl random", "box<->cyl coaxial", "hull<->hull", "hull<->table")


def family_queries(seed=11, per_family=110):
    """Part D: (family, query) lists.  Offsets are drawn around the hull's centroid (sigma 0.04 shallow, 0.005 deep), so most
    queries overlap; some do not, which is what the comparison of the penetrating flag needs."""
    rng = np.random.default_rng(seed)
    out = []
    for fam in FAMILIES:
        for k in range(per_family):
            pa = np.r_[rng.uniform(-0.5, 0.5, 3) + [0.5, 0, 0.35], rand_quat(rng)]
            if fam.startswith("hull<->cyl"):
                link = 2 + k % 5
                c = pa[:3] + Rot.from_quat(pa[3:]).apply(hull_verts(link).mean(0))
                pb = np.r_[c + rng.normal(0, 0.04 if fam.endswith("shallow") else 0.005, 3), rand_quat(rng)]
                q = (HULL, [link, 0, 0], pa, CYLZ, CYL, pb)
            elif fam == "sphere<->cyl":
                rb = Rot.from_quat(rand_quat(rng))
                # every fifth sphere sits at the cylinder's centre (every exit equally far in a whole circle of directions)
                off = np.zeros(3) if k % 5 == 0 else rb.apply(np.r_[rng.uniform(-0.05, 0.05, 2), rng.uniform(-0.2, 0.2)])
                q = (SPHERE, [0.02, 0, 0], np.r_[pa[:3], IDENT], CYLZ, CYL, np.r_[pa[:3] - off, rb.as_quat()])
            elif fam == "box<->cyl random":
                q = (BOX, CUBE_HALF, pa, CYLZ, CYL, np.r_[pa[:3] + rng.normal(0, 0.03, 3), rand_quat(rng)])
            elif fam == "box<->cyl coaxial":
                # the box's z axis on the cylinder's axis, the two rotated about it by a random angle: flat caps face to face
                rb = Rot.from_quat(pa[3:])
                spin = Rot.from_rotvec([0, 0, rng.uniform(-np.pi, np.pi)])
                pb = np.r_[pa[:3] + rb.apply([0, 0, rng.uniform(-0.21, 0.21)]), (rb * spin).as_quat()]
                q = (BOX, CUBE_HALF, pa, CYLZ, CYL, pb)
            elif fam == "hull<->hull":
                la, lb = int(rng.integers(1, 4)), int(rng.integers(3, 7))
                ra, rb = Rot.from_quat(pa[3:]), Rot.from_quat(rand_quat(rng))
                tb = pa[:3] + ra.apply(hull_verts(la).mean(0)) - rb.apply(hull_verts(lb).mean(0)) + rng.normal(0, 0.03, 3)
                q = (HULL, [la, 0, 0], pa, HULL, [lb, 0, 0], np.r_[tb, rb.as_quat()])
            else:
                link = 2 + k % 5
                ra = Rot.from_quat(pa[3:])
                s = _surface_point(rng, np.asarray(TABLE[1]))
                c = TABLE[2][:3] + s * (1.0 - rng.uniform(-0.02, 0.04) / np.abs(s).max())
                q = (HULL, [link, 0, 0], np.r_[c - ra.apply(hull_verts(link).mean(0)), pa[3:]], TABLE[0], TABLE[1], TABLE[2])
            out.append((fam, q))
    return out


def coaxial_closed_form(query):
    """Distance of a "box<->cyl coaxial" query in closed form: with the box on the cylinder's axis, core_A - core_B is a prism
    (a square rounded by the disc, times an interval of z), and the origin's distance to its boundary is the smaller of the radial
    exit -- box half + cylinder radius, through a side of the box -- and the axial one."""
    _, half, xa, _, cyl, xb = query
    off = Rot.from_quat(xb[3:]).inv().apply(xa[:3] - xb[:3])
    assert np.abs(off[:2]).max() < 1e-12
    hb, rc, hc = half[0] - MARGIN, cyl[0] - MARGIN, 0.5 * cyl[1] - MARGIN
    return -(min(hb + rc, hb + hc - abs(off[2])) + 2 * MARGIN)


EPA_CAP_RESIDUAL = 1.0e-5  # the project's constant: a search that stops at the cap with less than this to gain is not flagged


def oracle_census(oracle, queries):
    """The oracle's answer and the census of its EPA for every (label, query): a list of dicts with distance, penetrating, capped
    (iterations == 1001), and for penetrating queries expansions, at_cap, max_nc, degenerate_faces, max_face_slot."""
    rows = []
    for label, q in queries:
        r = oracle.closest(*q)
        row = dict(label=label, distance=r["distance"], penetrating=r["penetrating"], capped=r["iterations"] == 1001)
        if r["penetrating"]:
            row.update(expansions=oracle.last_epa_iterations(), **oracle.last_epa_census())
            row["at_cap"] = row["expansions"] >= EPA_CAP
        rows.append(row)
    return rows


def census_table(rows, labels=None):
    """Per label: queries, penetrating, expansion quantiles (min / median / p90 / max), at the cap, flagged, largest nc, degenerate
    faces, highest face slot -- as text lines for the verbose output."""
    lines = []
    for lab in labels or sorted({r["label"] for r in rows}):
        pen = [r for r in rows if r["label"] == lab and r["penetrating"]]
        n = sum(r["label"] == lab for r in rows)
        if not pen:
            lines.append(f"  {lab:20s} {n:4d} queries, none penetrating")
            continue
        ex = np.array([r["expansions"] for r in pen])
        lines.append(f"  {lab:20s} {n:4d} queries, {len(pen):4d} penetrating; expansions min/med/p90/max {ex.min()}/{int(np.median(ex))}/"
                     f"{int(np.quantile(ex, 0.9))}/{ex.max()}, <=4: {int((ex <= 4).sum())}, at cap {sum(r['at_cap'] for r in pen)}, "
                     f"flagged {sum(r['capped'] for r in pen)}, max nc {max(r['max_nc'] for r in pen)}, degenerate faces "
                     f"{sum(r['degenerate_faces'] for r in pen)}, top slot {max(r['max_face_slot'] for r in pen)}")
    return lines


def assert_census_conditions(rows):
    """The conditions part D sets for one run -- on the ORACLE's census, so that what the device is compared on is known to
    contain searches that stop at the cap, flagged ones, trivially short ones and enough overlap in every family."""
    pen = [r for r in rows if r["penetrating"]]
    assert sum(r["at_cap"] for r in pen) >= 20, "searches that stop at the 48-point cap"
    assert sum(r["capped"] for r in pen) >= 2, "searches flagged `capped`"
    assert sum(r["expansions"] <= 4 for r in pen) >= 20, "searches of at most 4 expansions"
    for fam in FAMILIES:
        assert sum(r["label"] == fam for r in pen) >= 50, fam


# ------------------------------------------------------------------------------------------------ step / refresh kernels (WORKBENCH)
DEEP = -(2 * MARGIN) - 1e-9  # a link distance below this is a real EPA depth: deeper than the margin sum


def per_body_distances(oracle, q, obst_pose, link):
    """oracle.closest of link `link` (2..6) at joint angles q against (obstacle, table, track): what link_dist_scope = WORKBENCH
    takes the minimum of (include/urgym.h)."""
    rot, pos = oracle.fk(q)
    pose = np.r_[pos[link], Rot.from_matrix(rot[link]).as_quat()]
    bodies = ((CYLZ, CYL, obst_pose), TABLE, TRACK)
    return np.array([oracle.closest(HULL, [link, 0, 0], pose, t, p, x)["distance"] for t, p, x in bodies])


def workbench_census(oracle, buf, cap=60):
    """Of the oracle's state `buf` (OracleEnv.buf after a step or refresh under WORKBENCH): which body supplies each deep link cell.
    Returns dict(deep, by_body [obstacle, table, track] (cells), envs_by_body (sets of envs), two_bodies_deep (cells in which two
    bodies are both deep: two EPA results meet in one cell), envs_multi_deep (envs with two or more deep links: one wave serves
    several marks), recompute_err).  The per-body recomputation covers the first `cap` deep cells; recompute_err is how far its
    minimum is from the cell (the bodies are queried one by one here, through a quaternion: not bitwise the same search)."""
    ld = buf["link_dist"]
    deep = ld < DEEP
    out = dict(deep=int(deep.sum()), by_body=[0, 0, 0], envs_by_body=[set(), set(), set()], two_bodies_deep=0,
               envs_multi_deep=int((deep.sum(0) >= 2).sum()), recompute_err=0.0)
    for i, n in list(zip(*np.nonzero(deep)))[:cap]:
        d = per_body_distances(oracle, buf["q"][:, n], np.r_[buf["obst_pos"][:, n], buf["obst_quat"][:, n]], i + 2)
        out["recompute_err"] = max(out["recompute_err"], abs(d.min() - ld[i, n]))
        out["by_body"][int(np.argmin(d))] += 1
        out["envs_by_body"][int(np.argmin(d))].add(int(n))
        out["two_bodies_deep"] += int((d < DEEP).sum() >= 2)
    return out


def refresh_workbench_state(oracle, n=48, seed=7):
    """Part G: joint angles that bend the arm down over the base -- shoulder lift in [-0.6, 0.9] puts the upper arm into the track
    and the forearm through the table top in about one pose of seven -- and, for every third env, the obstacle's centre inside
    one of that pose's links.  Returns the state dict for set_state / load_state (q, obst_start as xyz + rpy)."""
    rng = np.random.default_rng(seed)
    q = np.c_[rng.uniform(-np.pi, np.pi, n), rng.uniform(-0.6, 0.9, n), rng.uniform(-1.5, 1.5, n), rng.uniform(-2, 2, (n, 3))].T.copy()
    obst = np.c_[rng.uniform([0.5, -0.5, 0.25], [1.0, 0.5, 0.55], (n, 3)), rng.uniform(-2.6, 2.6, (n, 2)), np.zeros(n)]
    for i in range(0, n, 3):
        _, t = oracle.fk(q[:, i])
        link = 2 + (i // 3) % 5
        obst[i, :3] = 0.5 * (t[link] + t[min(link + 1, 6)]) + rng.normal(0, 0.01, 3)
    return {"q": q, "obst_start": obst.T.copy()}
