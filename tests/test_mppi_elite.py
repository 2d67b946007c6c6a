"""GPU tests (-m gpu) of elite samples and the adaptive std of the MPPI planner (include/urgym.h, "elite samples and an adaptive std";
DESIGN.md section 29): the two launches against their numpy restatements (ur_gym_amd.evaluation.mppi_elite_*, mppi_actions with an
array sigma) and against the plain launches they must equal, the three composed calls against the sequence of single calls they promise
to be and against the plain and guided calls where the options say "as before", every refusal, and DeviceMPPI's choice of entry point.

Shapes: K in {2, 3, 64, 65, 1000, 1024} with E in {1, 3} and H in {1, 3} on synthetic returns for the rank and the update; E K = 6 and
E K H = 585 (a ragged last workgroup of 256) for the sample; E = 3, K = 8, H = 3, I = 3, M = 3 for everything that steps.
"""
import ctypes as C

import numpy as np
import pytest

from mppi_elite_cases import LAM, LAYOUTS, RANK_SAMPLES, elite_actions, elite_counts, random_std, rank_returns
from test_mppi_collect import SHORT, assert_same_everything, assert_same_ring, close, guarded_replay, pattern_slots, stepped_loop
from test_mppi_guide import GUARD, OUTPUTS, STATE, Guarded, actor_path, check, critic_paths, guards_intact, make_vec, np_, refused, same_bits
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import DeviceMPPI, DeviceReplay, mppi_actions, mppi_elite_rank, mppi_elite_update, mppi_elite_weights

pytestmark = pytest.mark.gpu

E, H = 3, 3
K, ITERATIONS, ELITES = 8, 3, 3  # of everything that steps
SIGMA = 0.3
STD_MIN, STD_MAX = 0.05, 0.6
ADAPT_NAMES = tuple(name for name, _, _ in _abi.MPPI_ADAPT_FIELDS)
SHARED = ("new_mean", "mean", "action_out", "best_return", "nominal_return", "ess", "w")  # what the update and the elite update both write
GUIDED = dict(policy_samples=2, policy_sigma=0.2, terminal_value=True)


class GuardedElite(Guarded):
    """test_mppi_guide.Guarded with a urgym_mppi_adapt whose arrays lie between guard words as well (rank and elite only with `ranks`)."""

    def __init__(self, e, k, h, *, elites, adapt_std=0, std_min=STD_MIN, std_max=STD_MAX, ranks=True, **options):
        super().__init__(e, k, h, **options)
        A = _abi.MppiAdapt()
        A.elites, A.adapt_std, A.std_min, A.std_max = elites, adapt_std, std_min, std_max
        for name, ct, shape in _abi.MPPI_ADAPT_FIELDS:
            if ranks or name not in ("rank", "elite"):
                self._array(A, name, ct, shape(e, k, h))
        self.A = A


def guard(mppi):
    """test_mppi_guide.guard for a planner that may have a urgym_mppi_adapt: moves every array of a DeviceMPPI between guard words."""
    import torch

    full = {}
    owner = {name: mppi.struct() for name, _, _ in _abi.MPPI_FIELDS}
    owner.update({name: mppi.guide() for name, _, _ in _abi.MPPI_GUIDE_FIELDS})
    owner.update({name: mppi.adapt() for name in ADAPT_NAMES})
    types = {name: ct for name, ct, _ in _abi.MPPI_FIELDS + _abi.MPPI_GUIDE_FIELDS + _abi.MPPI_ADAPT_FIELDS}
    for name, t in list(mppi.buf.items()):
        raw = torch.full(((t.numel() + 2 * GUARD) * t.element_size(),), 0xA5, dtype=torch.uint8, device="cuda:0")
        full[name] = raw.view(t.dtype)
        mppi.buf[name] = full[name][GUARD:GUARD + t.numel()].view(t.shape)
        mppi.buf[name].zero_()
        setattr(owner[name], name, C.cast(mppi.buf[name].data_ptr(), C.POINTER(types[name])))
    return full


def same_values(a, b):
    """best_return is a maximum: of -0.0 and 0.0 the device's fold and numpy's max need not keep the same zero."""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------------------------------------ 1. the elite update
def launch_update(lib, env, g, elite=True):
    import torch

    call = lib.urgym_mppi_update_elite(env._h, C.byref(g.M), C.byref(g.A), env._stream()) if elite else lib.urgym_mppi_update(env._h, C.byref(g.M), env._stream())
    check(call, env)
    torch.cuda.synchronize()
    return {name: np_(t) for name, t in g.a.items()}


@pytest.fixture(scope="module")
def device():
    env = make_vec("UR5OriReach-v1", 1, 0)  # names the device; needs no reset
    yield env
    env.close()


@pytest.mark.parametrize("layout", range(len(LAYOUTS)))
@pytest.mark.parametrize("k", RANK_SAMPLES)
def test_elite_update_is_the_restatement_given_its_weights(device, k, layout):
    """For every M of the case list, at (E, H) = (3, 3), (1, 3), (3, 1), (1, 1): rank, elite, elite_count, threshold, new_mean, mean,
    action_out, ess, nominal_return and new_std are bitwise the restatement given the device's w (best_return by value: see same_values);
    w is within the plain update's bound of numpy's exp; parent 0 alone is its row at E = 3; with M == K every shared output is bitwise
    urgym_mppi_update's with shift 0 and 1; without rank and elite the other outputs are the same."""
    lib, worst = _native.lib(), 0.0
    all_ret, all_actions = rank_returns(k, layout), elite_actions(H, E, k, 40 + k)
    for m in elite_counts(k):
        rows = {}
        for e, h, shift in ((E, H, 1), (1, H, 1), (E, 1, 0), (1, 1, 0)):
            ret, actions = all_ret[:e * k], np.ascontiguousarray(all_actions[:h, :e * k])
            g = GuardedElite(e, k, h, elites=m, lam=LAM, shift=shift)
            g.put("ret", ret)
            g.put("actions", actions)
            got = launch_update(lib, device, g)
            case = (k, layout, m, e, h)
            assert g.guards_intact() and g.untouched(("eps", "g", "alive", "end_step", "success", "collided", "std", "policy_action", "value", "terminal")), case
            w = got["w"]
            want = dict(mppi_elite_rank(ret, k, m), **mppi_elite_update(ret, w, actions, shift, STD_MIN, STD_MAX))
            for key, value in want.items():
                if key == "best_return":
                    assert same_values(got[key], value), (case, key)
                else:
                    assert same_bits(got[key], value), (case, key, got[key], value)
            ref, _ = mppi_elite_weights(ret, LAM, k, m)
            ulps = np.abs(w - ref) / np.spacing(ref)
            worst = max(worst, float(ulps.max()))
            assert ulps.max() <= 3.0, (case, float(ulps.max()))  # the bound tests/test_mppi.py holds the plain weights to
            assert ((w > 0) == ((got["elite"] != 0) | ((got["elite_count"] == 0)[:, None] & (np.arange(k) == 0)))).all(), case
            rows[e, h] = got
            if m == k:  # the plain update on the same inputs, both shifts
                for s in (0, 1):
                    pair = [GuardedElite(e, k, h, elites=m, lam=LAM, shift=s) for _ in range(2)]
                    for x in pair:
                        x.put("ret", ret)
                        x.put("actions", actions)
                    elite, plain = launch_update(lib, device, pair[0]), launch_update(lib, device, pair[1], elite=False)
                    for key in SHARED:
                        assert same_bits(elite[key], plain[key]), (case, s, key)
                    assert pair[1].untouched(ADAPT_NAMES) and pair[1].guards_intact(), case
            if (e, h) == (E, H) and m == elite_counts(k)[-2]:  # rank and elite are optional: the same launch without them writes the same bits
                bare = GuardedElite(e, k, h, elites=m, lam=LAM, shift=shift, ranks=False)
                bare.put("ret", ret)
                bare.put("actions", actions)
                again = launch_update(lib, device, bare)
                assert set(got) - set(again) == {"rank", "elite"} and bare.guards_intact(), case
                for key in SHARED + ("new_std", "elite_count", "threshold"):
                    assert same_bits(again[key], got[key]), (case, key)
        for h in (H, 1):  # parent 0 alone equals its row at E = 3
            one, three = rows[1, h], rows[E, h]
            for key in ("new_mean", "mean", "new_std"):
                assert same_bits(one[key], three[key][:, :1]), (k, layout, m, h, key)
            for key in ("rank", "elite", "elite_count", "threshold", "action_out", "best_return", "nominal_return", "ess", "w"):
                assert same_bits(one[key], three[key][:1]), (k, layout, m, h, key)
    print(f"elite update K={k} layout={layout}: the device's exp against numpy's float64 exp, largest error {worst:.3f} ulp")


# ------------------------------------------------------------------------------------------------ 2. the adaptive sample
@pytest.mark.parametrize("e,k", [(3, 2), (3, 65)])
def test_adaptive_sample_is_the_sample_with_a_width_per_element(device, e, k):
    """E K = 6, and E K H = 585 lanes: two full workgroups of 256 and a ragged third.  With std filled with sigma, actions and eps are
    bitwise urgym_mppi_sample's; with a random std, actions are bitwise mppi_actions(std) on the device's eps, which is the same eps."""
    import torch

    lib = _native.lib()
    seed, draw, iteration = 0xC0FFEE1234, (1 << 32) - 1, 3
    rng = np.random.default_rng(e * k)
    mean = rng.uniform(-0.9, 0.9, (H, e, 6)).astype(np.float32)
    mean[:, 1, 0::2], mean[:, 1, 1::2] = 1.0, -1.0  # parent 1 at the bounds: the clamp acts

    def sample(std, adaptive=True):
        g = GuardedElite(e, k, H, elites=k, sigma=SIGMA, seed=seed)
        g.put("mean", mean)
        g.put("std", std)
        if adaptive:
            check(lib.urgym_mppi_sample_adaptive(device._h, C.byref(g.M), C.byref(g.A), draw, iteration, device._stream()), device)
        else:
            check(lib.urgym_mppi_sample(device._h, C.byref(g.M), draw, iteration, device._stream()), device)
        torch.cuda.synchronize()
        assert g.guards_intact() and g.untouched([n for n in g.a if n not in ("actions", "eps", "mean", "std")]), (e, k, adaptive)
        assert same_bits(np_(g.a["mean"]), mean) and same_bits(np_(g.a["std"]), std)
        return np_(g.a["actions"]), np_(g.a["eps"])

    flat = np.full((H, e, 6), SIGMA, np.float32)
    plain, adaptive = sample(flat, adaptive=False), sample(flat)
    assert same_bits(adaptive[0], plain[0]) and same_bits(adaptive[1], plain[1]) and plain[1][:, 1::k].all()
    std = random_std(H, e, k)
    actions, eps = sample(std)
    assert same_bits(eps, plain[1]) and not eps[:, ::k].any()
    assert same_bits(actions, mppi_actions(mean, eps, std)) and not same_bits(actions, plain[0])
    assert same_bits(actions[:, ::k], np.clip(mean, -1, 1))  # sample 0 is the nominal whatever its width
    assert same_bits(actions[0, :k, 0], np.full(k, mean[0, 0, 0], np.float32))  # a width of 0: the mean itself
    assert np.abs(actions).max() == 1.0 and (std == 25.0).any()  # the clamp acts: parent 1 sits at the bounds, one width is 25


# ------------------------------------------------------------------------------------------------ 3. the plan
def planner_pair(env_id, guided, *, elites=ELITES, adapt_std=True, iterations=ITERATIONS, std_min=STD_MIN, std_max=STD_MAX, **env_options):
    """A source that has been reset and a DeviceMPPI on it (with the golden actor and critics where `guided`), every array guarded.
    elites=None and adapt_std=False: the planner of before."""
    src = make_vec(env_id, E, 21, **env_options)
    src.reset(seed=21)
    learner = dict(actor=actor_path(env_id), critic=critic_paths(env_id), **GUIDED) if guided else {}
    mppi = DeviceMPPI(src, samples=K, horizon=H, sigma=SIGMA, lam=20.0, gamma=0.95, iterations=iterations, seed=8, keep_weights=True, elites=elites,
                      adapt_std=adapt_std, std_min=std_min, std_max=std_max, **learner)
    if guided:  # the single call urgym_actor_forward refuses a handle that has observed nothing (the composed calls do not ask)
        mppi.planner.reset(seed=5)
        mppi.planner._needs_reset = False
    return src, mppi, guard(mppi)


def single_calls_plan(lib, mppi, draw):
    """What urgym_mppi_plan_adaptive promises to be."""
    src, planner, M, A, G = mppi.env, mppi.planner, mppi.struct(), mppi.adapt(), mppi.guide()
    s = src._stream()
    shift, iterations = M.shift, M.iterations
    terminal = G is not None and (bool(G.terminal_value) or G.fail_cost > 0)

    def actor_forward():
        check(lib.urgym_actor_forward(planner._h, mppi.actor._a, C.c_void_p(mppi.buf["policy_action"].data_ptr()), s), planner)

    for i in range(iterations):
        check(lib.urgym_mppi_fanout(src._h, planner._h, C.byref(M), s), src)
        if A.adapt_std and i >= 1:
            mppi.buf["std"].copy_(mppi.buf["new_std"])  # on the same stream
            check(lib.urgym_mppi_sample_adaptive(src._h, C.byref(M), C.byref(A), draw, i, s), src)
        else:
            check(lib.urgym_mppi_sample(src._h, C.byref(M), draw, i, s), src)
        for h in range(H):
            if G is not None and G.policy_samples > 0:
                actor_forward()
                check(lib.urgym_mppi_guide_actions(planner._h, C.byref(M), C.byref(G), h, s), planner)
            check(lib.urgym_step(planner._h, C.c_void_p(mppi.buf["actions"][h].data_ptr()), s), planner)
            check(lib.urgym_mppi_score(planner._h, C.byref(M), h, s), planner)
        if G is not None and G.terminal_value:
            actor_forward()
            rows = _abi.CriticRows(None, None, None, G.policy_action)
            out = _abi.CriticOut(None, G.value, None)
            check(lib.urgym_critic_evaluate(planner._h, mppi.critic._c, C.byref(rows), E * M.samples, None, C.byref(out), s), planner)
        if terminal:
            check(lib.urgym_mppi_terminal(planner._h, C.byref(M), C.byref(G), s), planner)
        M.shift = shift if i == iterations - 1 else 0
        check(lib.urgym_mppi_update_elite(src._h, C.byref(M), C.byref(A), s), src)
        M.shift = shift


def assert_same_as_before(a, b, where):
    """`a` has a urgym_mppi_adapt, `b` has none: every buffer `b` has, the planner's and the source's bound buffers, bit for bit."""
    assert set(a.buf) - set(b.buf) == set(ADAPT_NAMES), where
    for key in b.buf:
        assert same_bits(np_(a.buf[key]), np_(b.buf[key])), (where, key)
    for key in STATE + OUTPUTS:
        assert same_bits(np_(a.planner.buf[key]), np_(b.planner.buf[key])), (where, "planner", key)
    for key in a.env.buf:
        assert same_bits(np_(a.env.buf[key]), np_(b.env.buf[key])), (where, "source", key)


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("env_id", ["UR5DynReach-v1", "UR5OriReach-v1"])
def test_plan_adaptive_is_its_single_calls(env_id, guided):
    import torch

    lib = _native.lib()
    (sa, a, fa), (sb, b, fb) = (planner_pair(env_id, guided, auto_reset=False) for _ in range(2))
    for draw in (0, 1):  # the second plan starts from the shifted mean of the first, and from sigma again
        action, diagnostics = a.plan(draw)
        single_calls_plan(lib, b, draw)
        torch.cuda.synchronize()
        assert_same_everything(a, b, (env_id, guided, draw))
        assert guards_intact(fa) and guards_intact(fb)
        assert same_bits(np_(action), np_(a.buf["new_mean"][0]))
        assert set(diagnostics) == {"best_return", "nominal_return", "ess", "elite_count", "threshold"} | ({"terminal"} if guided else set())
        got = {key: np_(t) for key, t in a.buf.items()}
        assert (got["elite_count"] == ELITES).all() and (got["elite"].sum(axis=1) == ELITES).all() and ((got["w"] > 0) == (got["elite"] != 0)).all()
        assert (got["ess"] >= 1).all() and (got["ess"] <= ELITES * (1 + 1e-12)).all() and (got["threshold"] <= got["best_return"]).all()
        assert same_bits(got["std"], np_(b.buf["std"])) and (got["std"] >= np.float32(STD_MIN)).all() and (got["std"] <= np.float32(STD_MAX)).all()
        assert not same_bits(got["std"], got["new_std"])  # std is what the last iteration sampled with: new_std of the one before it
        assert (got["std"] != np.float32(SIGMA)).any()  # ... and it was not sigma
    close(a, b, sa, sb)


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("mode", ["every sample an elite", "std pinned at sigma"])
def test_plan_adaptive_with_the_options_off_is_the_plan(mode, guided):
    """M == K and adapt_std off: urgym_mppi_plan_adaptive leaves every buffer as urgym_mppi_plan(_guided) leaves it.  adapt_std on with
    std_min == std_max == sigma: again the plain plan, bit for bit -- with the adaptive sample kernel running in iterations 1 and 2."""
    import torch

    env_id = "UR5DynReach-v1"
    options = dict(elites=K, adapt_std=False) if mode == "every sample an elite" else dict(elites=K, adapt_std=True, std_min=SIGMA, std_max=SIGMA)
    (sa, a, fa), (sb, b, fb) = planner_pair(env_id, guided, auto_reset=False, **options), planner_pair(env_id, guided, auto_reset=False, elites=None, adapt_std=False)
    assert a.adapt() is not None and b.adapt() is None
    for draw in (0, 1):
        a.plan(draw)
        b.plan(draw)
        torch.cuda.synchronize()
        assert_same_as_before(a, b, (mode, guided, draw))
        assert guards_intact(fa) and guards_intact(fb)
        finite = np.isfinite(np_(a.buf["ret"]).reshape(E, K)).sum(axis=1)
        assert same_bits(np_(a.buf["elite_count"]), finite.astype(np.int32))
        if options["adapt_std"]:
            assert (np_(a.buf["std"]) == np.float32(SIGMA)).all() and (np_(a.buf["new_std"]) == np.float32(SIGMA)).all()
        else:
            assert not np_(a.buf["std"]).any()  # never written
    close(a, b, sa, sb)


# ------------------------------------------------------------------------------------------------ 4. the closed loop and the collection
RECORD = ("action", "reward", "terminated", "truncated", "is_success")


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
def test_control_adaptive_is_plan_step_record(guided):
    """urgym_mppi_control_adaptive with T = 4 against record pass 0 and 4 x (plan_adaptive, step, record), with a source that auto-resets
    and a time limit of 3 steps (every env finishes inside the call); and against two calls of 2 + 2 steps."""
    import torch

    from ur_gym_amd.vector_env import _TORCH_DTYPE

    lib = _native.lib()
    T, env_id = 4, "UR5DynReach-v1"
    (sa, a, fa), (sb, b, fb), (sc, c, fc) = (planner_pair(env_id, guided, **SHORT) for _ in range(3))
    first = a.run(T, first_draw=10, record="all")
    torch.cuda.synchronize()
    first = {key: np_(v).copy() for key, v in first.items()}
    traj, rec = _abi.Trajectory(), {}
    for name, ct, shape in _abi.TRAJECTORY_FIELDS:
        rec[name] = torch.zeros(shape(T, E, sb.obs_dim, sb.goal_dim), dtype=_TORCH_DTYPE[ct], device="cuda:0")
        setattr(traj, name, C.cast(rec[name].data_ptr(), C.POINTER(ct)))
    assert set(rec) == set(first)
    M, A, G = b.struct(), b.adapt(), b.guide()
    check(lib.urgym_mppi_record(sb._h, C.byref(M), 0, T, C.byref(traj), sb._stream()), sb)
    for t in range(T):
        check(lib.urgym_mppi_plan_adaptive(sb._h, b.planner._h, C.byref(M), C.byref(A), C.byref(G) if guided else None, 10 + t, sb._stream()), sb)
        check(lib.urgym_step(sb._h, C.c_void_p(b.buf["action_out"].data_ptr()), sb._stream()), sb)
        check(lib.urgym_mppi_record(sb._h, C.byref(M), t + 1, T, C.byref(traj), sb._stream()), sb)
    halves = [c.run(2, first_draw=10, record=RECORD), c.run(2, first_draw=12, record=RECORD)]
    torch.cuda.synchronize()
    assert_same_everything(a, b, "control")
    assert_same_everything(a, c, "2 + 2")
    assert guards_intact(fa) and guards_intact(fb) and guards_intact(fc)
    for name in first:
        assert same_bits(first[name].view(np.uint8) if first[name].dtype == np.bool_ else first[name], np_(rec[name])), name
    for name in RECORD:
        assert same_bits(first[name], np.concatenate([np_(half[name]) for half in halves])), name
    finished = first["terminated"] | first["truncated"]
    assert finished[:3].any(axis=0).all() and first["episode_done"].all()  # the time limit of 3 steps: every env finished inside the call
    assert same_bits(first["action"][3], np_(a.buf["action_out"]))
    close(a, b, c, sa, sb, sc)


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
def test_collect_adaptive_is_the_python_stepped_loop(guided):
    """4 steps with explore_sigma = 0.3 into a ring of 3 slots (the call wraps) on a source that auto-resets with a time limit of 3 steps:
    ONE urgym_mppi_collect_adaptive against the Python-stepped loop (plan_adaptive, execute, step), and against 2 + 2 steps."""
    import torch

    env_id, capacity, steps, draw, sigma = "UR5DynReach-v1", 3, 4, 10, 0.3
    (sa, a, fa), (sb, b, fb), (sc, c, fc) = (planner_pair(env_id, guided, **SHORT) for _ in range(3))
    ra, ga = guarded_replay(sa, capacity)
    rc, gc = guarded_replay(sc, capacity)
    ra.collect_planned(a, steps, first_draw=draw, explore_sigma=sigma)
    want, finished = stepped_loop(b, capacity, 0, draw, steps, sigma)
    rc.collect_planned(c, 2, first_draw=draw, explore_sigma=sigma)
    rc.collect_planned(c, 2, first_draw=draw + 2, explore_sigma=sigma)
    torch.cuda.synchronize()
    assert (ra.cursor, ra.filled) == (rc.cursor, rc.filled) == (1, 3)
    assert_same_ring(ra.ring, want, (guided, "loop"))
    assert_same_everything(a, b, (guided, "loop"))
    assert_same_ring(ra.ring, rc.ring, (guided, "2 + 2"))
    assert_same_everything(a, c, (guided, "2 + 2"))
    assert all(guards_intact(f) for f in (fa, fb, fc, ga, gc))
    assert finished[:3].any(axis=0).all(), finished
    assert (np_(a.buf["elite_count"]) == ELITES).all()
    close(a, b, c, sa, sb, sc)


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
def test_control_and_collect_with_the_options_off_are_the_calls_of_before(guided):
    """M == K and adapt_std off: the trajectory of urgym_mppi_control_adaptive is urgym_mppi_control(_guided)'s and the ring of
    urgym_mppi_collect_adaptive is urgym_mppi_collect's, with every buffer they leave."""
    import torch

    env_id, steps, draw = "UR5DynReach-v1", 4, 10
    off, before = dict(elites=K, adapt_std=False, **SHORT), dict(elites=None, adapt_std=False, **SHORT)
    (sa, a, fa), (sb, b, fb) = planner_pair(env_id, guided, **off), planner_pair(env_id, guided, **before)
    ta, tb = a.run(steps, first_draw=draw, record="all"), b.run(steps, first_draw=draw, record="all")
    torch.cuda.synchronize()
    for key in tb:
        assert same_bits(np_(ta[key]), np_(tb[key])), (guided, key)
    assert_same_as_before(a, b, (guided, "control"))
    close(a, b, sa, sb)
    (sa, a, fa), (sb, b, fb) = planner_pair(env_id, guided, **off), planner_pair(env_id, guided, **before)
    ra, ga = guarded_replay(sa, 3)
    rb, gb = guarded_replay(sb, 3)
    ra.collect_planned(a, steps, first_draw=draw, explore_sigma=0.3)
    rb.collect_planned(b, steps, first_draw=draw, explore_sigma=0.3)
    torch.cuda.synchronize()
    assert_same_ring(ra.ring, rb.ring, (guided, "collect"))
    assert_same_as_before(a, b, (guided, "collect"))
    assert all(guards_intact(f) for f in (fa, fb, ga, gb))
    close(a, b, sa, sb)


# ------------------------------------------------------------------------------------------------ 5. the refusals
def test_every_refusal_launches_nothing():
    import torch

    from ur_gym_amd.evaluation import DeviceActor, DeviceCritic

    lib = _native.lib()
    env_id = "UR5DynReach-v1"
    src = make_vec(env_id, E, 1, auto_reset=True)
    src.reset(seed=1)
    fresh = make_vec(env_id, E, 1, auto_reset=True)  # has observed nothing
    planner = make_vec(env_id, E * K, 1, auto_reset=False)
    resetting = make_vec(env_id, E * K, 1, auto_reset=True)
    short = make_vec(env_id, E * K - 1, 1, auto_reset=False)
    ori = make_vec("UR5OriReach-v1", E * K, 1, auto_reset=False)
    actor, critic = DeviceActor.load(actor_path(env_id), planner), DeviceCritic.load(critic_paths(env_id), planner)
    source_actor = DeviceActor.load(actor_path(env_id), src)
    replay, ring_guards = guarded_replay(src, 4)
    torch.cuda.synchronize()
    before = {key: np_(planner.buf[key]).copy() for key in STATE + OUTPUTS}
    source_before = {key: np_(t).copy() for key, t in src.buf.items()}
    g = GuardedElite(E, K, H, elites=ELITES, adapt_std=1, iterations=2, policy_samples=2, policy_sigma=0.1, terminal_value=1, fail_cost=10.0, actor=actor, critic=critic)
    x = _abi.MppiExplore(0.3, 0, None)
    s = src._stream()
    names = ("urgym_mppi_sample_adaptive", "urgym_mppi_update_elite", "urgym_mppi_plan_adaptive", "urgym_mppi_control_adaptive", "urgym_mppi_collect_adaptive")
    composed = names[2:]

    def edited(struct, **fields):
        new = type(struct).from_buffer_copy(struct)
        for name, value in fields.items():
            setattr(new, name, value)
        return new

    def ref(p):
        return C.byref(p) if p is not None else None

    def calls(M=g.M, A=g.A, G=g.G, X=x, source=src, plan=planner, draw=0, steps=2, traj=None, ring=replay._ring, slot=0, iteration=0):
        sh, ph = getattr(source, "_h", None), getattr(plan, "_h", None)
        return {names[0]: lambda: lib.urgym_mppi_sample_adaptive(sh, ref(M), ref(A), draw, iteration, s),
                names[1]: lambda: lib.urgym_mppi_update_elite(sh, ref(M), ref(A), s),
                names[2]: lambda: lib.urgym_mppi_plan_adaptive(sh, ph, ref(M), ref(A), ref(G), draw, s),
                names[3]: lambda: lib.urgym_mppi_control_adaptive(sh, ph, ref(M), ref(A), ref(G), draw, steps, ref(traj), s),
                names[4]: lambda: lib.urgym_mppi_collect_adaptive(sh, ph, ref(M), ref(A), ref(G), ref(X), draw, steps, ref(ring), slot, s)}

    def every(*words, only=names, **fields):
        """Every entry point of `only` refuses the edit, naming itself and `words`; the source keeps the message."""
        for who, call in calls(**fields).items():
            if who in only:
                refused(call(), fields.get("source", src), who, *words)

    # everything the corresponding plain or guided call refuses
    for who, call in calls(source=None).items():
        refused(call(), None, "null handle")
    every("null planner handle", only=composed, plan=None)
    every("null urgym_mppi", M=None)
    for name, _, _ in _abi.MPPI_FIELDS[:-1]:
        every(f"urgym_mppi.{name} is null", M=edited(g.M, **{name: None}))
    for fields, word in ((dict(samples=1), "samples"), (dict(samples=1025), "samples"), (dict(horizon=0), "horizon"), (dict(horizon=65), "horizon"),
                         (dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"), (dict(num_parents=0), "num_parents"),
                         (dict(sigma=float("nan")), "sigma"), (dict(sigma=-0.5), "sigma"), (dict(lam=0.0), "lam"), (dict(lam=float("nan")), "lam"),
                         (dict(gamma=float("inf")), "gamma"), (dict(reserved0=1), "reserved"), (dict(reserved1=1), "reserved")):
        every(word, M=edited(g.M, **fields))
    every("the source has", only=composed, M=edited(g.M, num_parents=E + 1))
    every("auto_reset", only=composed, plan=resetting)
    every("num_parents * samples", only=composed, plan=short)
    every("urgym_config", only=composed, plan=ori)
    every("the planner has", only=composed, plan=src)
    for draw in (1 << 32, (1 << 64) - 1):
        every("2^32", only=(names[0],) + composed, draw=draw)
    every("2^32", only=composed[1:], draw=(1 << 32) - 1, steps=2)
    for iteration in (-1, 8):
        every("iteration", only=names[:1], iteration=iteration)
    for steps in (0, -1):
        every("num_steps", only=composed[1:], steps=steps)
    traj = _abi.Trajectory()
    summary = torch.zeros(E, dtype=torch.float64, device="cuda:0")
    traj.episode_return = C.cast(summary.data_ptr(), C.POINTER(C.c_double))
    every("episode_done", only=names[3:4], traj=traj)
    # the guide
    every("reserved0", only=composed, G=edited(g.G, reserved0=1))
    for p in (-1, K):
        every("policy_samples", only=composed, G=edited(g.G, policy_samples=p))
    every("actor is null", only=composed, G=edited(g.G, actor=None))
    every("critic is null", only=composed, G=edited(g.G, critic=None))
    every("actor is not an actor of the planner handle", only=composed, G=edited(g.G, actor=source_actor._a))
    for value in (float("nan"), float("inf"), -0.5):
        every("policy_sigma", only=composed, G=edited(g.G, policy_sigma=value))
        every("fail_cost", only=composed, G=edited(g.G, fail_cost=value))
    for name in ("policy_action", "value", "terminal"):
        every(f"{name} is null", only=composed, G=edited(g.G, **{name: None}))
    # the exploration, the ring and the source's state
    every("null urgym_mppi_explore", only=names[4:], X=None)
    every("reserved0", only=names[4:], X=edited(x, reserved0=1))
    for value in (float("nan"), float("inf"), -0.5):
        every("explore_sigma", only=names[4:], X=edited(x, explore_sigma=value))
    every("null ring", only=names[4:], ring=None)
    every("capacity_steps", only=names[4:], ring=edited(replay._ring, capacity_steps=0))
    for name, _, _, required in _abi.REPLAY_RING_FIELDS:
        if required:
            every("ring pointer is null", only=names[4:], ring=edited(replay._ring, **{name: None}))
    for slot in (-1, 4):
        every("first_slot", only=names[4:], slot=slot)
    every("observed", only=names[4:], source=fresh)
    # urgym_mppi_adapt
    every("null urgym_mppi_adapt", A=None)
    for m in (0, -1, K + 1):
        every("urgym_mppi_adapt.elites", A=edited(g.A, elites=m))
    for value in (float("nan"), float("inf"), -float("inf"), -0.5):
        every("urgym_mppi_adapt.std_min", A=edited(g.A, std_min=value))
        every("urgym_mppi_adapt.std_max", A=edited(g.A, std_min=0.0, std_max=value))
    every("std_min must not exceed std_max", A=edited(g.A, std_min=0.5, std_max=0.25))
    for name in ("std", "new_std", "elite_count", "threshold"):
        every(f"urgym_mppi_adapt.{name} is null", A=edited(g.A, **{name: None}))
    torch.cuda.synchronize()
    assert g.untouched() and g.guards_intact() and guards_intact(ring_guards) and pattern_slots(replay.ring, slice(None)) and not np_(summary).any()
    for key in STATE + OUTPUTS:
        assert same_bits(np_(planner.buf[key]), before[key]), key
    for key, want in source_before.items():
        assert same_bits(np_(src.buf[key]), want), key
    # DeviceMPPI says the same before it creates anything
    for bad in (dict(elites=0), dict(elites=K + 1), dict(adapt_std=True, std_min=-0.1), dict(adapt_std=True, std_min=0.7), dict(elites=2, std_max=float("nan"))):
        with pytest.raises(ValueError):
            DeviceMPPI(src, samples=K, horizon=H, **bad)
    close(actor, critic, source_actor, src, fresh, planner, resetting, short, ori)


# ------------------------------------------------------------------------------------------------ 6. DeviceMPPI picks the entry points
class Recorder:
    """Stands where an env's `lib` stands and notes the name of every planner entry point that is looked up."""

    def __init__(self, lib):
        self._lib, self.seen = lib, []

    def __getattr__(self, name):
        if name.startswith("urgym_mppi_"):
            self.seen.append(name)
        return getattr(self._lib, name)


ALL = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)


@pytest.mark.parametrize("options,suffix", [(dict(), ""), (dict(elites=ELITES), "_adaptive"), (dict(adapt_std=True, iterations=2), "_adaptive")],
                         ids=["as before", "elites", "adapt_std"])
def test_device_mppi_picks_the_entry_points(options, suffix):
    """plan, run, DeviceReplay.collect_planned and SACLearner.collect(planner=): a planner with elites= or adapt_std= calls the adaptive
    entry points, one without them the entry points it called before -- by symbol."""
    import torch

    from ur_gym_amd.training import SACLearner

    env = make_vec("UR5OriReach-v1", E, 21, **SHORT)
    env.reset(seed=21)
    learner = SACLearner(env, seed=5, hidden_width=32, batch_size=64, **ALL)
    mppi = DeviceMPPI(env, samples=K, horizon=2, sigma=SIGMA, lam=20.0, seed=8, **options)
    replay = DeviceReplay(env, 6)
    env.lib = spy = Recorder(env.lib)
    adaptive = bool(suffix)
    assert (mppi.adapt() is not None) == adaptive
    assert set(mppi.DIAGNOSTICS) == {"best_return", "nominal_return", "ess"} | ({"elite_count", "threshold"} if adaptive else set())
    assert DeviceMPPI.DIAGNOSTICS == ("best_return", "nominal_return", "ess")
    _, diagnostics = mppi.plan(0)
    assert set(diagnostics) == set(mppi.DIAGNOSTICS)
    mppi.run(2, first_draw=1, record=("reward",))
    replay.collect_planned(mppi, 2, first_draw=3, explore_sigma=0.1)
    learner.draw = 5
    learner.collect(replay, 2, planner=mppi, explore_sigma=0.1)
    torch.cuda.synchronize()
    if adaptive:
        assert spy.seen == ["urgym_mppi_plan_adaptive", "urgym_mppi_control_adaptive", "urgym_mppi_collect_adaptive", "urgym_mppi_collect_adaptive"], spy.seen
        m = options.get("elites", K)
        assert (np_(mppi.buf["elite_count"]) == m).all() and (np_(mppi.buf["elite"]).sum(axis=1) == m).all()
        assert np.isfinite(np_(mppi.buf["threshold"])).all()
        if options.get("adapt_std"):
            assert np_(mppi.buf["std"]).all() and (np_(mppi.buf["new_std"]) >= np.float32(0.05)).all() and (np_(mppi.buf["new_std"]) <= np.float32(SIGMA)).all()
    else:
        assert spy.seen == ["urgym_mppi_plan", "urgym_mppi_control", "urgym_mppi_collect", "urgym_mppi_collect"], spy.seen
    assert (replay.cursor, replay.filled, learner.env_steps, learner.draw) == (4, 4, 2, 7)
    assert np.abs(np_(replay.ring["action"][:4])).max() <= 1.0 and np_(replay.ring["action"][:4]).any()
    close(mppi, learner, env)
