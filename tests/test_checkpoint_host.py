"""CPU tests (-m "not gpu") of the checkpoint.

  * tests/unpack_harness.cpp, a stand-alone host program around urgym_pack_map.h and urgym_pack_host.h: the packing map run the other
    way, as the unpack kernels run it, for every env kind x hidden width in {32, 160, 256, 288, 512}; built a second time with
    -fsanitize=address,undefined and run as that program.
  * the ctypes mirrors of the three output structs against the header text and the C compiler's own layout, the new symbols, and the
    refusals that need no device.
  * the file: a synthetic state through ``checkpoint.write`` / ``checkpoint.read`` (``allow_pickle=False``) bitwise; a writer that dies
    midway leaves the previous file whole.
  * the mismatch errors of the ``load_state_dict`` methods, on objects that need no device (the ring and the monitor on a stand-in
    environment with CPU tensors, the learner's checks on a learner assembled without its device objects).
"""
import ctypes as C
import json
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ur_gym_amd import _abi, _native, checkpoint
from ur_gym_amd.evaluation import ACTOR_ARRAYS, CRITIC_ARRAYS, LOG_STD_ARRAYS, DeviceActor, DeviceCritic, DeviceMonitor, DeviceReplay
from ur_gym_amd.training import SAC_DEFAULTS, SACLearner, TorchActor, TorchTwinCritic

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
WIDTHS = (32, 160, 256, 288, 512)
NEW_SYMBOLS = ("urgym_actor_unpack", "urgym_critic_unpack")


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "unpack_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "urgym.h"), os.path.join(CSRC, "urgym_pack_map.h"), os.path.join(CSRC, "urgym_pack_host.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("unpack_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("unpack_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def check_harness_run(exe):
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr and "FAIL" not in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    lines = run.stdout.splitlines()
    assert lines[-1] == "ok 40"
    for n_in in (30, 32, 41, 47):
        for H in WIDTHS:
            for who, n in (("actor", n_in), ("actor-no-head", n_in), ("critic", n_in + 6)):
                assert any(l.startswith(f"{who} in={n} H={H} ") for l in lines), (who, n, H)
    HP, HT = 384, 12  # the sizes are the ones the layout promises (HP = H padded to 128, HT = HP / 32)
    assert f"actor in=47 H=288 floats={HT * 6 * 256 + HT * HT * 4 * 256 + 14 * HP + 16}" in lines
    assert f"critic in=53 H=288 floats={2 * (HT * 7 * 256 + HT * HT * 4 * 256 + 3 * HP + 4)}" in lines


def test_unpack_map_inverts_the_host_packing_loops(harness):
    check_harness_run(harness)


def test_unpack_harness_under_the_sanitizers(sanitized_harness):
    check_harness_run(sanitized_harness)


def test_output_structs_mirror_the_header(harness):
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    run = subprocess.run([harness, "layout"], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr
    layout = json.loads(run.stdout)
    mirrors = (("urgym_actor_params_out", _abi.ActorParamsOut, _abi.ActorParamsDev), ("urgym_q_network_out", _abi.QNetworkOut, _abi.QNetworkDev),
               ("urgym_critic_params_out", _abi.CriticParamsOut, _abi.CriticParamsDev))
    assert set(layout) == {name for name, _, _ in mirrors}
    for name, mirror, source in mirrors:
        body = hdr[hdr.index(f"typedef struct {name} {{"):hdr.index(f"}} {name};")]
        declared = re.findall(r"^\s*(float\*|int32_t|urgym_q_network_out)\s+(\w+)(?:\[2\])?;", body, flags=re.M)
        assert [n for _, n in declared] == [f for f, _ in mirror._fields_], name  # the header's order is the mirror's
        assert "const" not in body, name                                          # pointers that are written
        want = dict(layout[name])
        assert C.sizeof(mirror) == want.pop("sizeof") == C.sizeof(source), name
        assert {f: getattr(mirror, f).offset for f, _ in mirror._fields_} == want, name  # the C compiler's own offsets
        assert [f for f, _ in mirror._fields_] == [f for f, _ in source._fields_], name   # mirrors urgym_*_dev field for field
    assert dict(_abi.CriticParamsOut._fields_)["qf"] is _abi.QNetworkOut * 2
    assert _abi.ABI_VERSION == 4 and "#define URGYM_ABI_VERSION 4" in hdr  # added within version 4
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym
    assert lib.urgym_abi_version() == 4
    # the header states the contract and the round trip, and read_packed points at the new calls
    for text in ("ONE launch on `stream`", "written when the launch RUNS", "ROUND TRIP: urgym_*_unpack followed by urgym_*_load (tau == 1)",
                 "(32 to 512)", "are urgym_actor_unpack /"):
        assert text in hdr, text


def test_refusals_that_need_no_device():
    lib = _native.lib()
    assert lib.urgym_actor_unpack(None, None, C.byref(_abi.ActorParamsOut()), None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    assert lib.urgym_critic_unpack(None, None, C.byref(_abi.CriticParamsOut()), None) == _abi.ERR_ARG
    assert lib.urgym_actor_unpack(None, None, None, None) == _abi.ERR_ARG and lib.urgym_critic_unpack(None, None, None, None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    # `out` of parameters() is checked like the sources of load_parameters: these never reach the library
    cpu = torch.device("cpu")
    out = {k: torch.zeros(s) for k, s in zip(ACTOR_ARRAYS, ((32, 30), (32,), (32, 32), (32,), (6, 32), (6,)))}
    assert DeviceActor.check_parameters(out, 30, 32, cpu) is False
    with pytest.raises(ValueError, match="shape"):
        DeviceActor.check_parameters(out, 30, 64, cpu)
    with pytest.raises(ValueError, match="needs both"):
        DeviceActor.check_parameters(dict(out, log_std_weight=torch.zeros((6, 32))), 30, 32, cpu)
    with pytest.raises(ValueError, match="two Q-networks"):
        DeviceCritic.check_parameters([{}], 36, 32, cpu)


# ------------------------------------------------------------------------------------------------ the file
def words(rng, shape):
    """float32 of every kind: random words (NaN payloads, denormals, infinities among them), with -0.0f planted."""
    a = rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
    a.reshape(-1)[::5] = 0x80000000
    a.reshape(-1)[1::7] = 0x7FC00ABC
    a.reshape(-1)[2::11] = 0x00000003
    return a.view(np.float32)


def synthetic_state(rng):
    return dict(learner=dict(env_id="UR5DynReach-v1", hp=dict(gamma=0.95, tau=0.005, learning_rate=1e-4, device_entropy=True, batch_size=64),
                             seed=(1 << 63) + 5, actor={k: words(rng, (3, 4)) for k in ACTOR_ARRAYS},
                             critic=[{k: words(rng, (5,)) for k in CRITIC_ARRAYS} for _ in range(2)],
                             adam_state=dict(step=7, betas=(0.9, 0.999), eps=1e-8), entropy_state=None, best_mean=-float("inf")),
                replay=dict(cursor=3, ring=dict(terminated=rng.integers(0, 2, (4, 8)).astype(np.uint8), reward=words(rng, (4, 8)))),
                records=rng.integers(-(1 << 62), 1 << 62, (3, 9)), generator=rng.integers(0, 256, 5056).astype(np.uint8),
                doubles=rng.standard_normal(6), empty=np.zeros((0, 9), np.int64), scalar=np.float64(0.1), extra=dict(updates=12, note="x", flag=True, none=None))


def same_tree(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same_tree(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, list) and len(a) == len(b) and all(same_tree(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def test_file_round_trip_is_bitwise(tmp_path):
    state = synthetic_state(np.random.default_rng(3))
    path = tmp_path / "run.npz"
    checkpoint.write(path, state)
    assert not os.path.exists(checkpoint.temporary_name(path))  # renamed, not copied
    with np.load(path, allow_pickle=False) as z:  # plain arrays and one JSON string, nothing pickled
        assert checkpoint.META_KEY in z.files and all(z[k].dtype != object for k in z.files)
        assert z["learner/actor/mu_weight"].tobytes() == state["learner"]["actor"]["mu_weight"].tobytes()
        meta = json.loads(str(z[checkpoint.META_KEY][()]))
        assert meta["format"] == checkpoint.FORMAT and meta["state"]["extra"] == dict(updates=12, note="x", flag=True, none=None)
    got = checkpoint.read(path)
    want = dict(state, scalar=0.1)  # a numpy scalar comes back as the Python float of the same value
    want["learner"] = dict(state["learner"], adam_state=dict(step=7, betas=[0.9, 0.999], eps=1e-8))
    assert same_tree(want, got)
    assert got["learner"]["seed"] == (1 << 63) + 5 and got["learner"]["best_mean"] == -float("inf")
    # what the file cannot hold is refused when it is written, not found missing when it is read
    for bad in (dict(a=object()), dict(a=np.array([None])), {"a/b": 1}, {1: 2}):
        with pytest.raises(ValueError):
            checkpoint.flatten(bad)
    other = tmp_path / "actor.npz"
    np.savez(open(other, "wb"), x=np.zeros(3))
    with pytest.raises(ValueError, match="not a checkpoint"):
        checkpoint.read(other)


class DyingStream:
    """A binary file object that fails after `limit` bytes: a job killed, or a disk filled, in the middle of a save."""

    def __init__(self, name, mode, limit):
        self.f, self.left = open(name, mode), limit

    def write(self, data):
        data = bytes(data)
        if len(data) > self.left:
            self.f.write(data[:self.left])
            self.f.flush()
            self.left = 0
            raise OSError("the writer died")
        self.left -= len(data)
        return self.f.write(data)

    def __getattr__(self, name):
        return getattr(self.f, name)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.f.close()
        return False


def test_a_dying_writer_leaves_the_previous_file_whole(tmp_path):
    rng = np.random.default_rng(4)
    first, second = synthetic_state(rng), synthetic_state(rng)
    path = tmp_path / "run.npz"
    checkpoint.write(path, first)
    with pytest.raises(OSError, match="died"):
        checkpoint.write(path, second, opener=lambda name, mode: DyingStream(name, mode, 4000))
    tmp = checkpoint.temporary_name(path)
    assert os.path.exists(tmp) and 0 < os.path.getsize(tmp) <= 4000  # the unfinished file lies beside it
    assert same_tree(checkpoint.read(path), checkpoint.read(path)) and checkpoint.read(path)["replay"]["ring"]["reward"].tobytes() == first["replay"]["ring"]["reward"].tobytes()
    checkpoint.write(path, second)  # the next save starts the temporary file again and replaces the old one
    assert not os.path.exists(tmp)
    assert checkpoint.read(path)["replay"]["ring"]["reward"].tobytes() == second["replay"]["ring"]["reward"].tobytes()


# ------------------------------------------------------------------------------------------------ load_state_dict refusals
def stand_in_env(num_envs=8, env_id="UR5DynReach-v1", auto_reset=True):
    od, gd = _abi.OBS_DIMS[_abi.ENV_IDS[env_id]]
    return SimpleNamespace(env_id=env_id, num_envs=num_envs, obs_dim=od, goal_dim=gd, device=torch.device("cpu"), cfg=SimpleNamespace(auto_reset=auto_reset))


def fill_ring(replay, rng, cursor, filled):
    for name, t in replay.ring.items():
        if t.dtype == torch.uint8:
            t.copy_(torch.from_numpy(rng.integers(0, 2, tuple(t.shape)).astype(np.uint8)))
        else:
            t.copy_(torch.from_numpy(words(rng, tuple(t.shape))))
    replay.cursor, replay.filled = cursor, filled


def test_replay_state_dict_round_trip_and_refusals(tmp_path):
    rng = np.random.default_rng(6)
    for cursor, filled in ((3, 3), (2, 4), (0, 4), (0, 0), (1, 2)):  # growing, wrapped, full at 0, empty, not collected from slot 0
        a, b = DeviceReplay(stand_in_env(), 4), DeviceReplay(stand_in_env(), 4)
        fill_ring(a, rng, cursor, filled)
        fill_ring(b, rng, 1, 1)  # garbage: a load that does nothing is noticed
        path = tmp_path / "ring.npz"
        checkpoint.write(path, dict(replay=a.state_dict()))
        state = checkpoint.read(path)["replay"]
        assert all(v.shape[0] == filled for v in state["ring"].values())  # only the filled slots are written
        b.load_state_dict(state)
        assert (b.cursor, b.filled, b.oldest_slot) == (cursor, filled, a.oldest_slot)
        valid = [(a.oldest_slot + i) % 4 for i in range(filled)]
        for name, _, _, _ in _abi.REPLAY_RING_FIELDS:
            assert a.ring[name][valid].numpy().tobytes() == b.ring[name][valid].numpy().tobytes(), (name, cursor, filled)
    a = DeviceReplay(stand_in_env(), 4)
    fill_ring(a, rng, 2, 4)
    state = a.state_dict()
    before = {k: v.clone() for k, v in a.ring.items()}
    for other, match in ((DeviceReplay(stand_in_env(), 8), "capacity"), (DeviceReplay(stand_in_env(num_envs=16), 4), "num_envs"),
                         (DeviceReplay(stand_in_env(env_id="UR5ObsReach-v1"), 4), "obs_dim")):
        fill_ring(other, rng, 1, 1)
        kept = {k: v.clone() for k, v in other.ring.items()}
        with pytest.raises(ValueError, match=match):
            other.load_state_dict(state)
        assert (other.cursor, other.filled) == (1, 1) and all(torch.equal(kept[k].view(torch.uint8), other.ring[k].view(torch.uint8)) for k in kept)
    with pytest.raises(ValueError, match="reward"):
        a.load_state_dict(dict(state, ring=dict(state["ring"], reward=state["ring"]["reward"].astype(np.float64))))
    assert all(torch.equal(before[k].view(torch.uint8), a.ring[k].view(torch.uint8)) for k in before)
    # without the data the ring loads empty, at the saved cursor
    a.load_state_dict(a.state_dict(include_data=False))
    assert (a.cursor, a.filled, len(a)) == (2, 0, 0)
    with pytest.raises(ValueError, match="filled_steps"):
        a.check_args(a.capacity, filled_steps=a.filled)  # what sample_into asks before it launches: updates are refused until it has data


def test_monitor_state_dict_round_trip_and_refusals():
    rng = np.random.default_rng(7)
    a, b = DeviceMonitor(stand_in_env(), capacity=4), DeviceMonitor(stand_in_env(), capacity=4)
    for name, ct in _abi.MONITOR_STATE_FIELDS:
        a.state[name].copy_(torch.from_numpy(rng.integers(0, 100, 8).astype(np.dtype(ct))))
    a.records.copy_(torch.from_numpy(rng.integers(-(1 << 62), 1 << 62, (4, 9))))
    a.count, a.iterations = 3, 11
    arrays, tree = checkpoint.flatten(a.state_dict())
    b.load_state_dict(checkpoint.unflatten(arrays, json.loads(json.dumps(tree))))
    assert (b.count, b.iterations) == (3, 11) and torch.equal(a.records[:3], b.records[:3]) and not b.records[3:].any()
    assert all(a.state[k].numpy().tobytes() == b.state[k].numpy().tobytes() for k in a.state)
    for other, match in ((DeviceMonitor(stand_in_env(num_envs=16), capacity=4), "envs"), (DeviceMonitor(stand_in_env(), capacity=4, clear=False), "clear"),
                         (DeviceMonitor(stand_in_env(), capacity=2), "capacity")):
        with pytest.raises(ValueError, match=match):
            other.load_state_dict(a.state_dict())
        assert other.count == 0 and not other.records.any() and not any(v.any() for v in other.state.values())


def assembled_learner(**overrides):
    """A SACLearner's checkpoint-facing attributes without its device objects: what check_state_dict looks at."""
    hp = dict(SAC_DEFAULTS, hidden_width=32, batch_size=64, **overrides)
    env = stand_in_env()
    L = object.__new__(SACLearner)
    n_in = env.obs_dim + 2 * env.goal_dim
    torch.manual_seed(0)
    L.env, L.hp, L.seed, L.env_steps, L.draw = env, hp, 0, 0, 0
    L.actor, L.critic = TorchActor(n_in, 32), TorchTwinCritic(n_in + 6, 32)
    L.log_ent_coef = torch.zeros(1, requires_grad=True)
    L.adam_state = L.entropy_state = None
    L.target = SimpleNamespace(in_features=n_in + 6, hidden_width=32)
    return L


def learner_state(L):
    host = lambda w: {k: v.detach().numpy().copy() for k, v in w.items()}  # noqa: E731
    return dict(env_id=L.env.env_id, num_envs=L.env.num_envs, hp=dict(L.hp), seed=5, env_steps=3, draw=3, actor=host(L.actor.tensors()),
                critic=[host(w) for w in L.critic.tensors()], target=[host(w) for w in L.critic.tensors()], log_ent_coef=L.log_ent_coef.detach().numpy().copy(),
                adam_state=None, entropy_state=None)


def test_learner_mismatches_name_the_first_difference():
    L = assembled_learner()
    state = learner_state(L)
    plan, target = L.check_state_dict(state)
    assert len(plan) == 8 + 12 + 1 and len(target) == 2
    cases = [
        (dict(state, env_id="UR5ObsReach-v1"), "env_id is 'UR5ObsReach-v1'"),
        (dict(state, num_envs=16), "num_envs is 16"),
        (dict(state, hp=dict(state["hp"], gamma=0.99)), "gamma is 0.99"),
        (dict(state, hp=dict(state["hp"], hidden_width=64)), "hidden_width is 64"),
        (dict(state, hp=dict(state["hp"], device_entropy=True)), "device_entropy is True"),
        (dict(state, hp=dict(state["hp"], learning_rate=3e-4)), "learning_rate is 0.0003"),
        (dict(state, hp=dict(state["hp"], gamma=0.99, tau=0.5)), "gamma is 0.99"),  # the FIRST difference, in SAC_DEFAULTS' order
        (dict(state, adam_state=dict(step=1)), "adam_state is present in the checkpoint"),
        (dict(state, actor=dict(state["actor"], mu_bias=np.zeros(5, np.float32))), r"actor.mu_bias must be float32 \(6,\)"),
        (dict(state, actor={k: v for k, v in state["actor"].items() if k != "mu_bias"}), "actor holds"),
        (dict(state, log_ent_coef=np.zeros(1, np.float64)), "log_ent_coef must be float32"),
        (dict(state, target=[state["target"][0], dict(state["target"][1], q_4_weight=np.zeros(32, np.float32))]), r"target.qf1.q_4_weight must be float32 \(1, 32\)"),
    ]
    for bad, match in cases:
        with pytest.raises(ValueError, match=match):
            L.check_state_dict(bad)
    # the two a resumed run may set anew, and nothing else
    L.check_state_dict(dict(state, hp=dict(state["hp"], learning_rate=3e-4, learning_starts=7)), override=("learning_rate", "learning_starts"))
    with pytest.raises(ValueError, match="learning_starts is 7"):
        L.check_state_dict(dict(state, hp=dict(state["hp"], learning_rate=3e-4, learning_starts=7)), override=("learning_rate",))
    with pytest.raises(ValueError, match="only"):
        L.check_state_dict(state, override=("gamma",))
