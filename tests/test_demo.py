"""GPU tests (-m gpu) of the demonstration ring: urgym_replay_sample_mixed / DeviceReplay.sample_into(
demonstrations=), urgym_sac_policy_terms_cloned_masked / env.policy_terms_cloned_masked, urgym_sac_train_demonstrated /
env.sac_train(demonstrating=) and SACLearner(demonstrations=, demo_batch_size=, bc_demo_only=).

The gather is compared BIT FOR BIT with the numpy take at evaluation.mixed_entries and with urgym_replay_sample at the same position;
the masked terms with evaluation.policy_terms_cloned(row_mask=), urgym_sac_policy_terms_cloned and urgym_sac_policy_terms; ``train``
with the Python loop of ``collect`` and ``update`` on a twin made from the same seeds.  The shapes are the smallest that cross the
boundaries: envs of 8 (the learner's) and 3 (the demonstrations'), rings of 4 and 3 slots with both oldest slots nonzero, counts of 1,
65 and 130 rows with D at, one short of and one past a wave's 64 samples; the learner at hidden width 32, a batch of 65, 3 to 4 iterations.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import sac_bc_cases as bc
from sac_bc_cases import FLAGS, WEIGHT, same
from test_demo_host import MASKS, mask_of
from test_sac_bc import BC, BC_KEYS, FIRST_DRAW, LOSS_KEYS, BcSide, Calls, Case, M, SEED, UPDATE_SEED, assert_same_values, same_but_nan
from test_sac_train import ALL, bits, guarded, guards_intact
from ur_gym_amd import _abi, make_vec
from ur_gym_amd.evaluation import DeviceMPPI, DeviceReplay, mixed_entries, policy_terms_cloned, replay_indices
from ur_gym_amd.training import DEMO_DEFAULTS, SACLearner

pytestmark = pytest.mark.gpu

KINDS = ("UR5OriReach-v1", "UR5DynReach-v1")  # the narrowest and the widest rows
N_OWN, N_DEMO, CAP_OWN, CAP_DEMO = 8, 3, 4, 3
GATHER_CASES = ((1, 0), (1, 1), (65, 0), (65, 1), (65, 63), (65, 64), (65, 65), (130, 64), (130, 65), (130, 129))
FLOAT_FIELDS = [name for name, ct, _, _ in _abi.REPLAY_RING_FIELDS if ct is C.c_float]
BYTE_FIELDS = [name for name, ct, _, _ in _abi.REPLAY_RING_FIELDS if ct is C.c_uint8]
ALL_FIELDS = FLOAT_FIELDS + BYTE_FIELDS + ["index", "source"]
TORCH = {"index": torch.int64, "source": torch.uint8}


def guard_ring(replay):
    """Moves every ring tensor of `replay` between guard words (the struct follows); returns the (flat, view) pairs."""
    pairs = {}
    for name, ct, _, _ in _abi.REPLAY_RING_FIELDS:
        old = replay.ring[name]
        flat, view = guarded(tuple(old.shape), old.dtype, old.device)
        view.copy_(old)
        replay.ring[name] = view
        setattr(replay._ring, name, C.cast(view.data_ptr(), C.POINTER(ct)))
        pairs[name] = (flat, view)
    return pairs


def encode(replay, ring_id):
    """Every float and byte of the ring encodes (ring, entry = slot * N + env, field, column): a read from the wrong ring or entry shows
    in any column.  Floats stay below 2^24 (exact); bytes are ring * 96 + field * 32 + entry (entry < 32)."""
    n = replay.env.num_envs
    for f, name in enumerate(FLOAT_FIELDS):
        t = replay.ring[name]
        cols = int(np.prod(t.shape[2:])) if t.dim() > 2 else 1
        entry = np.arange(replay.capacity * n).reshape(replay.capacity, n, 1)
        v = (((ring_id * 64 + f) * 64 + entry) * 64 + np.arange(cols).reshape(1, 1, cols)).astype(np.float32)
        t.copy_(torch.from_numpy(v.reshape(tuple(t.shape))))
    for f, name in enumerate(BYTE_FIELDS):
        entry = np.arange(replay.capacity * n).reshape(replay.capacity, n)
        replay.ring[name].copy_(torch.from_numpy((ring_id * 96 + f * 32 + entry).astype(np.uint8)))


class Rings:
    """The learner's env and ring (8 envs, 4 slots) and the demonstrations' (3 envs, 3 slots) of one kind, every ring tensor guarded."""

    def __init__(self, kind):
        self.envs = [make_vec(kind, num_envs=n, seed=3 + i, auto_reset=True) for i, n in enumerate((N_OWN, N_DEMO))]
        for e in self.envs:
            e.reset(seed=3)
        self.own, self.demo = DeviceReplay(self.envs[0], CAP_OWN), DeviceReplay(self.envs[1], CAP_DEMO)
        self.guards = {f"{w}.{k}": v for w, r in (("own", self.own), ("demo", self.demo)) for k, v in guard_ring(r).items()}
        self.env = self.envs[0]

    def synthetic(self):
        encode(self.own, 0), encode(self.demo, 1)
        self.own.cursor, self.own.filled = 1, 4    # oldest_slot 1
        self.demo.cursor, self.demo.filled = 1, 2  # oldest_slot 2: the two valid slots wrap
        assert self.own.oldest_slot == 1 and self.demo.oldest_slot == 2
        return self

    def sides(self):
        return tuple((r.oldest_slot, r.filled, r.env.num_envs, r.capacity) for r in (self.own, self.demo))

    def outputs(self, count, fields=ALL_FIELDS):
        env = self.env
        shapes = {name: tuple(shape(1, 1, env.obs_dim, env.goal_dim)[2:]) for name, _, shape, _ in _abi.REPLAY_RING_FIELDS}
        out = {}
        for k in fields:
            dtype = TORCH.get(k, torch.uint8 if k in BYTE_FIELDS else torch.float32)
            out[k] = guarded((count,) + shapes.get(k, ()), dtype, env.device, fill=0x55 if dtype == torch.uint8 else (-7 if dtype == torch.int64 else float("nan")))
        return out

    def mixed(self, count, D, seed, draw, fields=ALL_FIELDS):
        out = self.outputs(count, fields)
        self.own.sample_into({k: v[1] for k, v in out.items()}, seed, draw, demonstrations=(self.demo, D))
        return out

    def plain(self, count, seed, draw):
        out = self.outputs(count, [k for k in ALL_FIELDS if k != "source"])
        self.own.sample_into({k: v[1] for k, v in out.items()}, seed, draw)
        return out

    def expected(self, count, D, seed, draw):
        own, demo = self.sides()
        index, source = mixed_entries(seed, draw, count, own, D, demo)
        want = dict(index=index, source=source.astype(np.uint8))
        for name in FLOAT_FIELDS + BYTE_FIELDS:
            a, b = (r.ring[name].cpu().numpy().reshape((r.capacity * r.env.num_envs,) + tuple(r.ring[name].shape[2:])) for r in (self.own, self.demo))
            rows = np.empty((count,) + a.shape[1:], dtype=a.dtype)
            rows[source], rows[~source] = b[index[source]], a[index[~source]]
            want[name] = rows
        return want

    def intact(self):
        return guards_intact(self.guards)

    def close(self):
        for e in self.envs:
            e.close()


def host(out):
    return {k: v[1].cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ 1. the gather
@pytest.mark.parametrize("kind", KINDS)
def test_mixed_gather_on_synthetic_rings(kind):
    r = Rings(kind).synthetic()
    seed, draw = 0xC0FFEE1234, (1 << 40) + 9
    rows_at = {}
    for count, D in GATHER_CASES:
        where = (kind, count, D)
        out = r.mixed(count, D, seed, draw)
        again = r.mixed(count, D, seed, draw)  # a repeat
        other = r.mixed(count, D, seed, draw + 1)  # a second launch on the same stream, another draw
        plain = r.plain(count, seed, draw)
        torch.cuda.synchronize(r.env.device)
        got, want, base = host(out), r.expected(count, D, seed, draw), host(plain)
        for k in ALL_FIELDS:
            assert np.array_equal(bits(got[k]), bits(want[k])), (where, k)  # bitwise the numpy take at mixed_entries
            assert np.array_equal(bits(host(again)[k]), bits(got[k])), (where, k, "repeat")
        assert np.array_equal(got["source"], (np.arange(count) < D).astype(np.uint8)), where
        for k in base:  # rows >= D are urgym_replay_sample's at the same position; with D = 0 every output is
            assert np.array_equal(bits(got[k][D:]), bits(base[k][D:])), (where, k, "plain rows")
        if D:  # a demonstration row's floats name ring 1, every other row's ring 0
            assert (got["observation"][:D, 0] >= 64 ** 3).all() and (got["observation"][D:, 0] < 64 ** 3).all(), where
        if count > 1:
            assert not np.array_equal(host(other)["index"], got["index"]), where
        assert np.array_equal(host(other)["index"], r.expected(count, D, seed, draw + 1)["index"]), where
        for pairs in (out, again, other, plain):
            assert guards_intact(pairs) is None, where
        rows_at[(count, D)] = got
    for k in ALL_FIELDS:  # row i is the same at count 65 and 130
        assert np.array_equal(bits(rows_at[(65, 64)][k]), bits(rows_at[(130, 64)][k][:65])), k
        assert np.array_equal(bits(rows_at[(65, 65)][k]), bits(rows_at[(130, 65)][k][:65])), k
    # a batch with only some outputs given writes only those (the absent ones have no tensor at all), the same bits
    for fields in (("action", "source"), ("next_observation", "terminated"), ("index",), ("reward", "is_success", "desired_goal")):
        out = r.mixed(130, 65, seed, draw, fields)
        torch.cuda.synchronize(r.env.device)
        for k in fields:
            assert np.array_equal(bits(host(out)[k]), bits(rows_at[(130, 65)][k])), (fields, k)
        assert guards_intact(out) is None, fields
    assert r.intact() is None
    r.close()


@pytest.mark.parametrize("kind", KINDS)
def test_mixed_gather_on_collected_rings(kind):
    """Policy collection into one ring and the planner's collection into the other, both past their capacity."""
    r = Rings(kind)
    learner = SACLearner(r.envs[0], seed=SEED, hidden_width=32, batch_size=M, learning_starts=0, **ALL)
    learner.collect(r.own, CAP_OWN + 1)
    mppi = DeviceMPPI(r.envs[1], samples=5, horizon=2, sigma=0.3, lam=20.0, gamma=0.95, seed=8)
    r.demo.collect_planned(mppi, CAP_DEMO + 2, first_draw=0, explore_sigma=0.1)
    assert r.own.oldest_slot == 1 and r.demo.oldest_slot == 2 and r.own.filled == CAP_OWN and r.demo.filled == CAP_DEMO
    for count, D in ((65, 17), (130, 65), (65, 65), (65, 0)):
        out = r.mixed(count, D, 21, 5)
        torch.cuda.synchronize(r.env.device)
        got, want = host(out), r.expected(count, D, 21, 5)
        for k in ALL_FIELDS:
            assert np.array_equal(bits(got[k]), bits(want[k])), (kind, count, D, k)
        assert guards_intact(out) is None
    assert np.abs(r.demo.ring["action"].cpu().numpy()).max() > 0 and r.intact() is None
    mppi.close(), learner.close(), r.close()


def test_every_refusal_of_the_mixed_gather_leaves_the_outputs_unchanged():
    r = Rings(KINDS[0]).synthetic()
    env, lib, count = r.env, r.env.lib, 65
    out = r.outputs(count)
    batch = _abi.ReplayBatch()
    for name, ct, _, _ in _abi.REPLAY_RING_FIELDS:
        setattr(batch, name, C.cast(out[name][1].data_ptr(), C.POINTER(ct)))
    batch.index = C.cast(out["index"][1].data_ptr(), C.POINTER(C.c_int64))
    source = out["source"][1].data_ptr()

    def ring_of(replay, **over):
        ring = _abi.ReplayRing.from_buffer_copy(replay._ring)
        for k, v in over.items():
            setattr(ring, k, v)
        return ring

    def call(ring=None, oldest=None, filled=None, n=count, b=batch, demo="default", demo_ring=None, **d):
        ring = ring_of(r.own) if ring is None else ring
        if demo == "default":
            fields = dict(num_envs=N_DEMO, oldest_slot=r.demo.oldest_slot, filled_steps=r.demo.filled, count=17)
            fields.update(d)
            demo = C.byref(_abi.ReplayDemonstrations(ring_of(r.demo) if demo_ring is None else demo_ring, **fields))
        return lib.urgym_replay_sample_mixed(env._h, C.byref(ring) if ring is not False else None, r.own.oldest_slot if oldest is None else oldest,
                                             r.own.filled if filled is None else filled, 1, 2, n, C.byref(b) if b is not None else None, demo, source, env._stream())

    no_flags = ring_of(r.demo, truncated=None)
    cases = [
        # everything urgym_replay_sample refuses
        ("null ring", dict(ring=False), b"null ring"), ("capacity", dict(ring=ring_of(r.own, capacity_steps=0)), b"capacity_steps"),
        ("reserved0", dict(ring=ring_of(r.own, reserved0=1)), b"reserved0"), ("ring pointer", dict(ring=ring_of(r.own, action=None)), b"required ring pointer"),
        ("filled 0", dict(filled=0), b"filled_steps"), ("filled > C", dict(filled=CAP_OWN + 1), b"filled_steps"), ("oldest", dict(oldest=CAP_OWN), b"oldest_slot"),
        ("oldest < 0", dict(oldest=-1), b"oldest_slot"), ("count 0", dict(n=0), b"count"), ("null batch", dict(b=None), b"null batch"),
        ("empty batch", dict(b=_abi.ReplayBatch()), b"no output"), ("flags of own ring", dict(ring=ring_of(r.own, is_success=None)), b"does not keep it"),
        # the demonstrations' own
        ("null demo", dict(demo=None), b"null demonstrations"), ("demo capacity", dict(demo_ring=ring_of(r.demo, capacity_steps=0)), b"demonstrations: ring.capacity_steps"),
        ("demo capacity < 0", dict(demo_ring=ring_of(r.demo, capacity_steps=-3)), b"demonstrations: ring.capacity_steps"),
        ("demo reserved0", dict(demo_ring=ring_of(r.demo, reserved0=1)), b"demonstrations: urgym_replay_ring.reserved0"),
        ("demo pointer", dict(demo_ring=ring_of(r.demo, next_desired_goal=None)), b"demonstrations: a required ring pointer"),
        ("demo terminated", dict(demo_ring=ring_of(r.demo, terminated=None)), b"demonstrations: a required ring pointer"),
        ("num_envs 0", dict(num_envs=0), b"num_envs"), ("num_envs < 0", dict(num_envs=-1), b"num_envs"), ("demo oldest", dict(oldest_slot=CAP_DEMO), b"demonstrations: oldest_slot"),
        ("demo oldest < 0", dict(oldest_slot=-1), b"demonstrations: oldest_slot"), ("demo filled 0", dict(filled_steps=0), b"demonstrations: filled_steps"),
        ("demo filled > C", dict(filled_steps=CAP_DEMO + 1), b"demonstrations: filled_steps"), ("D < 0", dict(count=-1), b"demonstrations: count"),
        ("D > count", dict(count=count + 1), b"demonstrations: count"), ("demo flags", dict(demo_ring=no_flags), b"demonstration ring does not keep it"),
    ]
    for what, kw, expect in cases:
        rc = call(**kw)
        assert rc == _abi.ERR_ARG and expect in lib.urgym_last_error(env._h), (what, rc, lib.urgym_last_error(env._h))
    torch.cuda.synchronize(env.device)
    got = host(out)
    assert all(np.isnan(got[k]).all() for k in FLOAT_FIELDS) and all((got[k] == 0x55).all() for k in BYTE_FIELDS + ["source"]) and (got["index"] == -7).all()
    # a demonstration ring without the flags serves a batch that does not ask for them
    b2 = _abi.ReplayBatch.from_buffer_copy(batch)
    b2.truncated = b2.is_success = None
    assert call(b=b2, demo_ring=ring_of(r.demo, truncated=None, is_success=None)) == 0 and call() == 0  # and the good structs are good
    torch.cuda.synchronize(env.device)
    want = r.expected(count, 17, 1, 2)
    assert all(np.array_equal(bits(host(out)[k]), bits(want[k])) for k in ALL_FIELDS) and guards_intact(out) is None
    # the binding's own refusals
    for bad in (dict(demonstrations=(r.own, 1)), dict(demonstrations=(r.demo, count + 1)), dict(demonstrations=(r.demo, -1)), dict(demonstrations=(r.demo, 1), n_steps=2, gamma=0.9),
                dict(demonstrations=(DeviceReplay(r.envs[1], 2), 1))):
        with pytest.raises(ValueError):
            r.own.sample_into({k: v[1] for k, v in out.items()}, 1, 2, **bad)
    other = make_vec(KINDS[1], num_envs=2, seed=1, auto_reset=True)
    with pytest.raises(ValueError, match="another env kind is out of scope"):
        r.own.sample_into({k: v[1] for k, v in out.items()}, 1, 2, demonstrations=(DeviceReplay(other, 2), 1))
    other.close(), r.close()


# ------------------------------------------------------------------------------------------------ 2. the masked terms
@pytest.fixture(scope="module")
def env():
    e = make_vec("UR5OriReach-v1", num_envs=64, seed=3, auto_reset=True)
    e.reset(seed=3)
    yield e
    e.close()


class MaskedCase(Case):
    def masked(self, mask, scale_by_q, q_filter, d_action="d_action"):
        t = self.g.t
        self.mask = guarded((self.count,), torch.uint8, self.env.device)
        self.mask[1].copy_(torch.from_numpy(mask))
        self.env.policy_terms_cloned_masked(t["ent_coef"], self.count, row_mask=self.mask[1], **self.args(d_action), action_pi=t["action_pi"], action_data=t["action_data"],
                                            weight=WEIGHT, bc_scale=1.0 / self.count, scale_by_q=scale_by_q, q_filter=q_filter, bc_loss_out=t["bc_loss"],
                                            bc_weight_out=t["bc_weight"], bc_rows_out=self.rows[1])


@pytest.mark.parametrize("count", (1, 65, 1025, 65536))
def test_masked_terms_are_the_restatement_bitwise(env, count):
    c = MaskedCase(env, count)
    c.plain()
    torch.cuda.synchronize(env.device)
    plain = {k: c.g.host("plain_" + k) for k in ("d_action", "critic_loss", "actor_loss")}
    for kind in (MASKS if count < 65536 else ("prefix64", "scattered")):  # the cap once, on the two masks that mix
        mask = mask_of(kind, count)
        for scale_by_q, q_filter in FLAGS:
            where = (count, kind, scale_by_q, q_filter)
            want = bc.restate(c.x, count, scale_by_q, q_filter, row_mask=mask)
            c.masked(mask, scale_by_q, q_filter)
            got = c.assert_is(want, where)
            assert guards_intact({"mask": c.mask}) is None and np.array_equal(c.mask[1].cpu().numpy(), mask), where
            cloned = want["cloned"]
            assert not cloned[mask == 0].any() and same(got["d_action"][~cloned], plain["d_action"][~cloned]), where
            assert same(got["critic_loss"], plain["critic_loss"]) and same(got["actor_loss"], plain["actor_loss"]), where
            if kind == "ones":  # bitwise urgym_sac_policy_terms_cloned
                c.call(scale_by_q, q_filter)
                full = c.outputs()
                assert all(same(got[k], full[k]) for k in got if k != "bc_rows") and got["bc_rows"][0] == full["bc_rows"][0], where
            if kind == "zeros":  # bitwise urgym_sac_policy_terms, bc_loss +0.0, rows 0, bc_weight still written
                assert same(got["d_action"], plain["d_action"]) and got["bc_rows"][0] == 0, where
                assert same(got["bc_loss"], np.zeros(1, np.float32)) and same(got["bc_weight"], np.full(1, bc.restate(c.x, count, scale_by_q, q_filter)["bc_weight"])), where


def test_masked_terms_excluded_nan_and_in_place(env):
    count = 65
    for kind in ("prefix1", "prefix64", "scattered"):
        mask = mask_of(kind, count)
        clean = bc.inputs(count)
        c = MaskedCase(env, count)
        bad = clean["action_data"].copy()
        bad[mask == 0] = np.nan  # every row the mask excludes
        c.g.set("action_data", bad)
        c.x = dict(c.x, action_data=bad)
        for scale_by_q, q_filter in FLAGS:
            want = bc.restate(clean, count, scale_by_q, q_filter, row_mask=mask)  # the clean inputs' outputs: the NaN reaches none
            c.masked(mask, scale_by_q, q_filter)
            got = c.assert_is(want, (kind, scale_by_q, q_filter))
            assert np.isfinite(got["d_action"]).all() and np.isfinite(got["bc_loss"][0])
    c = MaskedCase(env, 1025)  # d_action_out aliasing dqmin_da
    mask = mask_of("scattered", 1025)
    want = bc.restate(c.x, 1025, True, True, row_mask=mask)
    c.masked(mask, True, True, d_action="dqmin_da")
    torch.cuda.synchronize(env.device)
    assert same(c.g.host("dqmin_da"), want["d_action"]) and np.isnan(c.g.host("d_action")).all() and c.rows[1].item() == want["bc_rows"]
    assert c.g.guards_intact() and guards_intact({"rows": c.rows, "mask": c.mask}) is None


def test_masked_terms_refusals(env):
    lib, count = env.lib, 65
    c = MaskedCase(env, count)
    t = c.g.t
    fptr = lambda x: C.cast(x.data_ptr(), C.POINTER(C.c_float))  # noqa: E731
    good_a = dict(count=count, reserved0=0, scale=-1.0 / count, ent_coef=fptr(t["ent_coef"]), dqmin_da=fptr(t["dqmin_da"]), d_action_out=fptr(t["d_action"]),
                  q=fptr(t["q"]), y=fptr(t["y"]), critic_loss_out=fptr(t["critic_loss"]), log_prob=fptr(t["log_prob"]), q_min=fptr(t["q_min"]),
                  actor_loss_out=fptr(t["actor_loss"]))
    good_b = dict(action_pi=fptr(t["action_pi"]), action_data=fptr(t["action_data"]), weight=WEIGHT, bc_scale=1.0 / count, scale_by_q=1, q_filter=1,
                  bc_loss_out=fptr(t["bc_loss"]), bc_weight_out=fptr(t["bc_weight"]), bc_rows_out=C.cast(c.rows[1].data_ptr(), C.POINTER(C.c_int32)), reserved0=0)
    mask = torch.ones(count, dtype=torch.uint8, device=env.device)
    cases = [("null mask", {}, {}, None, b"null row_mask"), ("null clone", {}, None, mask.data_ptr(), b"null clone args")]
    cases += [(f"args {k}", {k: v}, {}, mask.data_ptr(), e) for k, v, e in (("count", 0, b"count"), ("reserved0", 1, b"reserved0"), ("y", None, b"half given"),
                                                                               ("ent_coef", None, b"ent_coef"), ("scale", float("nan"), b"scale"))]
    cases += [("no upstream", dict(dqmin_da=None, d_action_out=None), {}, mask.data_ptr(), b"all three groups")]
    cases += [(f"clone {k}", {}, {k: v}, mask.data_ptr(), e) for k, v, e in (("action_pi", None, b"is null"), ("bc_rows_out", None, b"is null"), ("weight", -1.0, b"weight"),
                                                                                ("bc_scale", float("inf"), b"bc_scale"), ("q_filter", 2, b"0 or 1"), ("reserved0", 1, b"reserved0"))]
    cases += [("aliased", dict(d_action_out=fptr(t["action_data"])), {}, mask.data_ptr(), b"d_action_out is action_pi or action_data")]
    for what, a_over, b_over, m, expect in cases:
        a = _abi.SacPolicyArgs(**dict(good_a, **a_over))
        b = None if b_over is None else C.byref(_abi.SacCloneArgs(**dict(good_b, **b_over)))
        rc = lib.urgym_sac_policy_terms_cloned_masked(env._h, C.byref(a), b, m, env._stream())
        assert rc == _abi.ERR_ARG and expect in lib.urgym_last_error(env._h) and b"urgym_sac_policy_terms_cloned_masked" in lib.urgym_last_error(env._h), (what, rc)
    kw = dict(c.args(), action_pi=t["action_pi"], action_data=t["action_data"], weight=WEIGHT, bc_scale=1.0 / count, scale_by_q=True, q_filter=True,
              bc_loss_out=t["bc_loss"], bc_weight_out=t["bc_weight"], bc_rows_out=c.rows[1])
    for bad in (None, mask[:-1], mask.float(), mask.cpu(), mask.repeat(2)[::2]):
        with pytest.raises(ValueError, match="row_mask"):
            env.policy_terms_cloned_masked(t["ent_coef"], count, row_mask=bad, **kw)
    got = c.outputs()
    assert all(np.isnan(got[k]).all() for k in got if k != "bc_rows") and got["bc_rows"][0] == -7  # nothing was launched, nothing written
    env.policy_terms_cloned_masked(t["ent_coef"], count, row_mask=mask.bool(), **kw)  # a bool mask counts as uint8
    c.assert_is(bc.restate(c.x, count, True, True), "after the refusals")


# ------------------------------------------------------------------------------------------------ 3. the learner
D_CASES = (0, 17, 65)


class DemoSide(BcSide):
    """test_sac_bc's BcSide with a demonstration ring: a second env of 3 envs whose ring of 3 slots a planner filled past its capacity
    (oldest slot 2), the same bits whichever side it is.  D = None is the learner without the option (the ring is still made)."""

    def __init__(self, D, env_id="UR5OriReach-v1", seeds=0, fill=True, **over):
        self.env_d = make_vec(env_id, num_envs=N_DEMO, seed=41, auto_reset=True, max_episode_steps=3)
        self.env_d.reset(seed=41)
        self.replay_d = DeviceReplay(self.env_d, CAP_DEMO)
        if fill:
            mppi = DeviceMPPI(self.env_d, samples=5, horizon=2, sigma=0.3, lam=20.0, gamma=0.95, seed=9)
            self.replay_d.collect_planned(mppi, CAP_DEMO + 2, first_draw=0, explore_sigma=0.1)
            mppi.close()
        else:
            self.replay_d.cursor, self.replay_d.filled = 2, 3
        option = {} if D is None else dict(demonstrations=self.replay_d, demo_batch_size=D)
        super().__init__(env_id, seeds=seeds, **option, **over)

    def close(self):
        super().close()
        self.env_d.close()


def assert_same_sides(a, b, what, skip=(), last=True):
    sa, sb = a.state(), b.state()
    assert sa.keys() == sb.keys(), what
    assert sum(k.startswith("param:") for k in sa) == 8 + 12 and sum(k.startswith("moment:") for k in sa) == 2 * (8 + 12)
    for k in sa:
        if not k.startswith(skip):
            assert np.array_equal(bits(sa[k]), bits(sb[k])), (what, k)
    assert a.counters() == b.counters(), (what, a.counters(), b.counters())
    for k, t in a.replay_d.ring.items():  # nobody writes the demonstrations
        assert np.array_equal(bits(t), bits(b.replay_d.ring[k])), (what, "demonstrations", k)
    if last:
        la, lb = a.learner.last_update, b.learner.last_update
        assert sorted(la) == sorted(lb), (what, sorted(la), sorted(lb))
        for k in la:
            assert la[k].shape == lb[k].shape and np.array_equal(bits(la[k]), bits(lb[k])), (what, "last_update", k)


def values(got, n):
    """A train() result as the list loop() returns."""
    return [{k: got[k][u] for k in got if k != "plan_stats"} for u in range(n)]


@pytest.mark.parametrize("D", D_CASES)
def test_update_is_the_sequence_of_single_calls(D):
    s = DemoSide(D, **BC, bc_demo_only=True)
    lr = s.learner
    lr.collect(s.replay, CAP_DEMO + 2)
    assert s.replay.oldest_slot != 0 and s.replay_d.oldest_slot == 2
    for draw in range(2):
        own, demo = ((r.oldest_slot, r.filled, r.env.num_envs, r.capacity) for r in (s.replay, s.replay_d))
        rings = [{k: v.cpu().numpy().copy() for k, v in r.ring.items()} for r in (s.replay, s.replay_d)]
        losses = lr.update(s.replay, UPDATE_SEED, draw)
        torch.cuda.synchronize(s.env.device)
        last, es = lr.last_update, lr.entropy_state
        h = {k: v.cpu().numpy() for k, v in last.items()}
        index, source = mixed_entries(UPDATE_SEED, draw, M, own, D, demo)
        assert np.array_equal(h["source"], source.astype(np.uint8)), draw
        action = np.where(source[:, None], rings[1]["action"].reshape(-1, 6)[np.where(source, index, 0)], rings[0]["action"].reshape(-1, 6)[np.where(source, 0, index)])
        assert same(h["action_data"], action), draw  # the mixed gather at the plain call's (seed, draw)
        want = policy_terms_cloned(es["ent_coef"].cpu().numpy()[0], dqmin_da=h["dqmin_da"], scale=-1.0 / M, q=h["q"], y=h["y"], log_prob=h["log_prob"], q_min=h["q_min"],
                                   action_pi=h["action_pi"], action_data=h["action_data"], weight=BC["bc_weight"], bc_scale=1.0 / M, scale_by_q=True, q_filter=True,
                                   row_mask=h["source"])
        assert same(lr.actor_d_action.cpu().numpy(), want["d_action"]), draw
        assert same(losses["critic_loss"].cpu().numpy(), want["critic_loss"]) and same(losses["actor_loss"].cpu().numpy(), want["actor_loss"]), draw
        assert same(h["bc_loss"], np.full(1, want["bc_loss"])) and same(h["bc_weight"], np.full(1, want["bc_weight"])) and h["bc_rows"][0] == want["bc_rows"], draw
        assert want["bc_rows"] <= D and not want["cloned"][D:].any(), draw
        print(f"D {D} update {draw}: cloned {want['bc_rows']} of {D} demonstration rows, bc_loss {h['bc_loss'][0]!r}")
    s.close()


CASES = {"D0": (0, {}), "D17": (17, {}), "D65": (65, {}), "clipping": (17, dict(max_grad_norm=1e-2)), "normalize": (17, dict(normalize=True)),
         "planner_cloned_demo_only": (17, dict(planner=True, bc_demo_only=True, **BC))}


@pytest.mark.parametrize("case", list(CASES))
def test_train_equals_the_python_loop_bit_for_bit(case):
    D, over = CASES[case]
    iterations = 3 if "planner" in case else 4
    a, b = DemoSide(D, **over), DemoSide(D, **over)
    want = a.loop(iterations, 1, 2, FIRST_DRAW)
    got = b.train(iterations, 1, 2, FIRST_DRAW)
    torch.cuda.synchronize(a.env.device)
    assert len(want) == 2 * (iterations - 1), case
    for u, w in enumerate(want):
        for k in w:
            assert np.array_equal(bits(got[k][u]), bits(w[k])), (case, u, k)
    assert_same_sides(a, b, case)
    assert np.array_equal(b.learner.last_update["source"].cpu().numpy(), (np.arange(M) < D).astype(np.uint8)), case
    if "planner" in case:
        assert_same_values(want, got, case)
        assert (got["bc_rows"].cpu().numpy() <= D).all(), case
    a.close(), b.close()


def test_split_calls_and_d_zero_against_the_learner_without_the_option():
    a, b = DemoSide(17), DemoSide(17)
    whole = a.train(4, 1, 2, FIRST_DRAW)
    first = b.train(2, 1, 2, FIRST_DRAW)
    second = b.train(2, 1, 2, FIRST_DRAW + 2)
    torch.cuda.synchronize(a.env.device)
    for k in LOSS_KEYS:
        assert np.array_equal(bits(whole[k]), bits(torch.cat([first[k], second[k]]))), k
    assert_same_sides(a, b, "2 + 2 iterations")
    a.close(), b.close()
    for over in ({}, dict(BC, bc_demo_only=False)):
        # D = 0 through the new calls leaves the bits of a learner without the option: train and the loop of update alike
        zero, none, loop_zero = DemoSide(0, **over), DemoSide(None, **over), DemoSide(0, **over)
        g0, g1 = zero.train(4, 1, 2, FIRST_DRAW), none.train(4, 1, 2, FIRST_DRAW)
        want = loop_zero.loop(4, 1, 2, FIRST_DRAW)
        torch.cuda.synchronize(zero.env.device)
        assert sorted(g0) == sorted(g1)
        for k in g0:
            assert np.array_equal(bits(g0[k]), bits(g1[k])), k
            assert all(np.array_equal(bits(g0[k][u]), bits(w[k])) for u, w in enumerate(want)), k
        assert_same_sides(zero, none, "D = 0 against no option", last=False)
        assert_same_sides(zero, loop_zero, "D = 0, train against the loop")
        assert "source" in zero.learner.last_update and "source" not in none.learner.last_update and not zero.learner.last_update["source"].any()
        # D = 17 is another computation
        other = DemoSide(17, **over)
        g2 = other.train(4, 1, 2, FIRST_DRAW)
        assert not np.array_equal(bits(g2["critic_loss"]), bits(g0["critic_loss"]))
        for s in (zero, none, loop_zero, other):
            s.close()


NEW_SYMBOLS = ("urgym_replay_sample_mixed", "urgym_sac_policy_terms_cloned_masked", "urgym_sac_train_demonstrated")


def test_calls_with_and_without_the_option(tmp_path):
    seen = {}
    for label, D, over in (("plain", None, {}), ("cloned", None, BC), ("demo", 17, {}), ("demo_cloned", 17, BC), ("demo_only", 17, dict(BC, bc_demo_only=True))):
        s = DemoSide(D, **over)
        with Calls(s.env) as calls:
            s.learner.collect(s.replay, 4)
            s.learner.update(s.replay, UPDATE_SEED, 0)
            del calls.names[:]
            s.learner.update(s.replay, UPDATE_SEED, 1)
            update = list(calls.names)
            s.train(1, 0, 2, 2)
            seen[label] = (update, list(calls.names))
        if D is None:  # its checkpoint holds no new key
            path = tmp_path / f"{label}.npz"
            s.learner.save(path, replay=s.replay)
            assert not set(DEMO_DEFAULTS) & set(s.learner.state_dict()["hp"])
            with np.load(path, allow_pickle=False) as z:
                assert not any("demo" in k for k in z.files) and "demo" not in str(z["__checkpoint__"][()])
        s.close()
    swap = lambda names, pairs: [pairs.get(n, n) for n in names]  # noqa: E731
    # a learner without the option makes the calls it made: neither new symbol, the entry points of before
    for label, entry in (("plain", "urgym_sac_train"), ("cloned", "urgym_sac_train_cloned")):
        assert not set(NEW_SYMBOLS) & set(seen[label][1]) and seen[label][1][-1] == entry and seen[label][0].count("urgym_replay_sample") == 1
    # with it: the same calls in the same order, but for the ones that are replaced
    assert seen["demo"][0] == swap(seen["plain"][0], {"urgym_replay_sample": "urgym_replay_sample_mixed"})
    assert seen["demo_cloned"][0] == swap(seen["cloned"][0], {"urgym_replay_sample": "urgym_replay_sample_mixed"})
    assert seen["demo_only"][0] == swap(seen["cloned"][0], {"urgym_replay_sample": "urgym_replay_sample_mixed", "urgym_sac_policy_terms_cloned": "urgym_sac_policy_terms_cloned_masked"})
    assert all(seen[k][1][-1] == "urgym_sac_train_demonstrated" for k in ("demo", "demo_cloned", "demo_only"))


def test_save_and_load_continue_bit_for_bit(tmp_path):
    over = dict(BC, bc_demo_only=True)
    a, b = DemoSide(17, **over), DemoSide(17, **over)
    a.train(4, 1, 2, FIRST_DRAW)
    for _ in range(2):
        a.learner.update(a.replay, UPDATE_SEED, FIRST_DRAW + 6 + _)
    b.train(4, 1, 2, FIRST_DRAW)
    path, ring_path = tmp_path / "run.npz", tmp_path / "demos.npz"
    b.learner.save(path, replay=b.replay, demonstrations=b.replay_d, extra=dict(update_draw=FIRST_DRAW + 6))
    b.replay_d.save(ring_path)
    assert {k: b.learner.state_dict()["hp"][k] for k in DEMO_DEFAULTS} == dict(demo_batch_size=17, bc_demo_only=True)
    b.close()
    one = DemoSide(None, seeds=100, fill=False, **BC)  # a learner without the option refuses the file
    with pytest.raises(ValueError, match="demonstrations is present in the checkpoint"):
        one.learner.load(path, replay=one.replay)
    with pytest.raises(ValueError, match="demo_batch_size is 17 in the checkpoint, None here"):
        one.learner.load(path, replay=one.replay, demonstrations=one.replay_d)
    one.close()
    for wrong, match in ((dict(over, bc_demo_only=False), "bc_demo_only is True in the checkpoint, False here"), (over, "demo_batch_size is 17 in the checkpoint, 18 here")):
        other = DemoSide(18 if wrong is over else 17, seeds=100, fill=False, **wrong)
        with pytest.raises(ValueError, match=match):
            other.learner.load(path, replay=other.replay, demonstrations=other.replay_d)
        with pytest.raises(ValueError, match="demonstrations is present in the checkpoint"):
            other.learner.load(path, replay=other.replay)
        other.close()
    c = DemoSide(17, seeds=100, fill=False, **over)  # rebuilt from other seeds, the demonstration ring empty of data
    for t in list(c.replay.ring.values()) + list(c.replay_d.ring.values()):
        t.fill_(1)
    extra = c.learner.load(path, replay=c.replay, demonstrations=c.replay_d)
    for _ in range(2):
        c.learner.update(c.replay, UPDATE_SEED, extra["update_draw"] + _)
    torch.cuda.synchronize(a.env.device)
    assert_same_sides(a, c, "save, load, two more updates", skip=("grad:",))
    d = DeviceReplay(c.env_d, CAP_DEMO)  # the ring alone, from its own file
    d.load_file(ring_path)
    assert (d.cursor, d.filled) == (a.replay_d.cursor, a.replay_d.filled) and all(np.array_equal(bits(t), bits(a.replay_d.ring[k])) for k, t in d.ring.items())
    a.close(), c.close()


def test_every_refusal_of_the_training_call():
    s = DemoSide(17, **BC)
    env, lib, lr = s.env, s.env.lib, s.learner
    lr.collect(s.replay, 4)
    tr = lr._train_binding(s.replay)
    L = tr["binding"].struct
    before = {k: bits(v).copy() for k, v in s.state().items()}
    losses = torch.full((3, 2), float("nan"), device=env.device)
    for i, name in enumerate(_abi.SAC_LEARNER_LOSSES):
        setattr(L, name, C.cast(losses[i].data_ptr(), C.POINTER(C.c_float)))
    S = _abi.SacSchedule(s.replay.cursor, s.replay.filled, s.replay.capacity, 1, 0, 2, 0, 0, 0, 0, 1)
    source = torch.full((M,), 0x55, dtype=torch.uint8, device=env.device)
    bc_out = [torch.zeros(2, device=env.device), torch.zeros(2, device=env.device), torch.zeros(2, dtype=torch.int32, device=env.device)]
    cloning = _abi.SacCloning(0.5, 0, 0, 0, C.cast(bc_out[0].data_ptr(), C.POINTER(C.c_float)), C.cast(bc_out[1].data_ptr(), C.POINTER(C.c_float)),
                              C.cast(bc_out[2].data_ptr(), C.POINTER(C.c_int32)))

    def call(dem="default", cloning=None, schedule=S, extra=(None,) * 7, **over):
        if dem == "default":
            d = s.replay_d.demonstrations_struct(17)
            fields = dict(source=C.cast(source.data_ptr(), C.POINTER(C.c_uint8)), clone_demonstrations_only=0, reserved0=0)
            for k, v in over.items():
                if k in fields:
                    fields[k] = v
                elif k.startswith("ring_"):
                    setattr(d.ring, k[5:], v)
                else:
                    setattr(d, k, v)
            dem = C.byref(_abi.SacDemonstrating(d, **fields))
        return lib.urgym_sac_train_demonstrated(env._h, C.byref(L), C.byref(schedule), dem, None if cloning is None else C.byref(cloning), *extra, env._stream())

    idle = _abi.SacSchedule(s.replay.cursor, s.replay.filled, s.replay.capacity, 1, 0, 2, 0, 1, 0, 0, 1)  # one idle iteration: a call that holds no update
    cases = [
        ("null demonstrating", dict(dem=None), b"null demonstrating"), ("reserved0", dict(reserved0=1), b"urgym_sac_demonstrating.reserved0"),
        ("D > M", dict(count=M + 1), b"D > M"), ("D < 0", dict(count=-1), b"demonstrations: count"), ("null source", dict(source=None), b"source is null"),
        ("clone only without cloning", dict(clone_demonstrations_only=1), b"needs cloning"), ("clone only 2", dict(clone_demonstrations_only=2, cloning=cloning), b"0 or 1"),
        ("num_envs", dict(num_envs=0), b"num_envs"), ("oldest", dict(oldest_slot=CAP_DEMO), b"demonstrations: oldest_slot"), ("filled", dict(filled_steps=0), b"demonstrations: filled_steps"),
        ("ring capacity", dict(ring_capacity_steps=0), b"capacity_steps"), ("ring reserved0", dict(ring_reserved0=1), b"reserved0"), ("ring pointer", dict(ring_reward=None), b"required ring pointer"),
        ("refused without an update too", dict(schedule=idle, num_envs=0), b"num_envs"), ("reserved0 without an update", dict(schedule=idle, reserved0=1), b"reserved0"),
        # what the call with the same options and no demonstrations refuses
        ("cloning weight", dict(cloning=_abi.SacCloning(-1.0, 0, 0, 0, cloning.bc_loss, cloning.bc_weight, cloning.bc_rows)), b"weight"),
        ("temper without planning", dict(extra=(None, C.byref(_abi.MppiTemper()), None, None, None, None, None)), b"need planning"),
        ("schedule", dict(schedule=_abi.SacSchedule(s.replay.cursor, s.replay.filled, s.replay.capacity + 1, 1, 0, 2, 0, 0, 0, 0, 1)), b"capacity_steps"),
    ]
    for what, kw, expect in cases:
        rc = call(**kw)
        err = lib.urgym_last_error(env._h)
        assert rc == _abi.ERR_ARG and expect in err and b"urgym_sac_train_demonstrated" in err, (what, rc, err)
    assert call(schedule=idle, source=None) == 0  # zero updates need no source
    torch.cuda.synchronize(env.device)
    assert torch.isnan(losses).all() and (source == 0x55).all()  # nothing was launched, nothing written
    after = s.state()
    assert all(np.array_equal(before[k], bits(after[k])) for k in before)
    assert call(cloning=cloning, clone_demonstrations_only=1) == 0  # and the good structs are good
    torch.cuda.synchronize(env.device)
    assert not torch.isnan(losses).any() and np.array_equal(source.cpu().numpy(), (np.arange(M) < 17).astype(np.uint8)) and (bc_out[2] <= 17).all()
    for name in _abi.SAC_LEARNER_LOSSES:
        setattr(L, name, None)
    # the binding's own refusals
    good = dict(first_slot=s.replay.cursor, filled_steps=s.replay.filled, num_iterations=1, steps_per_iteration=0, updates_per_iteration=2)
    for bad in (dict(replay=s.replay, count=1, source=source), dict(replay=s.replay_d, count=M + 1, source=source), dict(replay=s.replay_d, count=1, source=source[:-1]),
                dict(replay=s.replay_d, count=1, source=source, clone_only=True), dict(replay=s.replay_d, count=1, source=source, clone_only=1),
                dict(replay=s.replay_d, count=1, source=source, other=1), dict(replay=DeviceReplay(s.env_d, 2), count=1, source=source)):
        with pytest.raises(ValueError):
            env.sac_train(tr["binding"], losses[0], losses[1], losses[2], demonstrating=bad, **good)
    with pytest.raises(ValueError, match="out of scope"):
        env.sac_train(tr["binding"], losses[0], losses[1], losses[2], demonstrating=dict(replay=s.replay_d, count=1, source=source),
                      hindsight=dict(n_sampled_goal=4, strategy="future", horizon=3), **good)
    s.close()
