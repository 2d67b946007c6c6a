"""CPU tests (-m "not gpu") of the weight reload.

  * tests/pack_harness.cpp, a stand-alone host program: the packing map of the device pack kernels (urgym_pack_map.h) run lane by
    lane on the host against the host packing loops the library creates actors and critics with (urgym_pack_host.h), for every env
    kind x hidden width in {32, 160, 256, 288, 512}; the blend against the three-operation float32 formula at tau = 0.005 and 1.
  * the ctypes mirrors of the new structs, the shape / dtype / device / key checks of load_parameters, and evaluation.polyak.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import ACTOR_ARRAYS, CRITIC_ARRAYS, LOG_STD_ARRAYS, DeviceActor, DeviceCritic, polyak

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
EXE = os.path.join(HERE, "_build", "pack_harness")
NEW_SYMBOLS = ("urgym_actor_load", "urgym_critic_load", "urgym_actor_read_packed", "urgym_critic_read_packed")
WIDTHS = (32, 160, 256, 288, 512)


@pytest.fixture(scope="module")
def harness_output():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    src = os.path.join(HERE, "pack_harness.cpp")
    deps = [src, os.path.join(CSRC, "urgym_pack_map.h"), os.path.join(CSRC, "urgym_pack_host.h"), os.path.join(ROOT, "include", "urgym.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", EXE, src])
    run = subprocess.run([EXE], capture_output=True, text=True)
    return run.returncode, run.stdout


def test_pack_map_equals_the_host_packing_loops(harness_output):
    rc, out = harness_output
    assert rc == 0 and "FAIL" not in out, out[-2000:]
    lines = out.splitlines()
    assert lines[-1] == "ok 40"
    for n_in in (30, 32, 41, 47):
        for H in WIDTHS:
            assert any(l.startswith(f"actor in={n_in} H={H} ") for l in lines), (n_in, H)
            assert any(l.startswith(f"critic in={n_in + 6} H={H} ") for l in lines), (n_in, H)
    # the sizes the harness reports are the ones the layout promises (HP = H padded to 128, HT = HP / 32)
    HP, HT = 384, 12
    assert f"actor in=47 H=288 floats={HT * 6 * 256 + HT * HT * 4 * 256 + 14 * HP + 16}" in lines
    assert f"critic in=53 H=288 floats={2 * (HT * 7 * 256 + HT * HT * 4 * 256 + 3 * HP + 4)}" in lines


def test_weight_structs_mirror_the_header():
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    ctype = {"const float*": C.POINTER(C.c_float), "int32_t": C.c_int32}

    def fields(struct):
        body = hdr[hdr.index(f"typedef struct {struct}"):hdr.index(f"}} {struct};")]
        return re.findall(r"^\s*(const float\*|int32_t|urgym_q_network_dev)\s+(\w+)(\[2\])?;", body, flags=re.M)

    got = fields("urgym_actor_params_dev")
    assert [(n, ctype[t]) for t, n, _ in got] == list(_abi.ActorParamsDev._fields_) and len(got) == 11
    assert [n for _, n, _ in got[3:]] == list(_abi.ACTOR_DEV_ARRAYS)
    got = fields("urgym_q_network_dev")
    assert [(n, ctype[t]) for t, n, _ in got] == list(_abi.QNetworkDev._fields_) and len(got) == 6
    got = fields("urgym_critic_params_dev")
    assert got[-1] == ("urgym_q_network_dev", "qf", "[2]")
    assert [(n, ctype[t]) for t, n, _ in got[:-1]] == list(_abi.CriticParamsDev._fields_[:-1]) and len(got) == 4
    assert _abi.CriticParamsDev._fields_[-1][1] is _abi.QNetworkDev * 2
    # three int32 and then pointers: the compiler pads to 8, and so does ctypes
    assert _abi.ActorParamsDev.w0.offset == 16 and C.sizeof(_abi.ActorParamsDev) == 16 + 8 * 8
    assert _abi.CriticParamsDev.qf.offset == 16 and C.sizeof(_abi.CriticParamsDev) == 16 + 2 * 6 * 8
    assert _abi.ABI_VERSION == 4 and "#define URGYM_ABI_VERSION 4" in hdr  # added within version 4
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
        assert re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym  # one line, starting with int
    assert lib.urgym_abi_version() == 4
    assert "urgym_actor_load replaces the head" in hdr  # set_log_std points to the new call


def _actor_tensors(n_in, H, head=True, device="cpu"):
    shapes = dict(zip(ACTOR_ARRAYS + LOG_STD_ARRAYS, ((H, n_in), (H,), (H, H), (H,), (6, H), (6,), (6, H), (6,))))
    keys = ACTOR_ARRAYS + (LOG_STD_ARRAYS if head else ())
    return {k: torch.zeros(shapes[k], dtype=torch.float32, device=device) for k in keys}


def _critic_tensors(n_in, H, device="cpu"):
    shapes = dict(zip(CRITIC_ARRAYS, ((H, n_in), (H,), (H, H), (H,), (1, H), (1,))))
    return [{k: torch.zeros(sh, dtype=torch.float32, device=device) for k, sh in shapes.items()} for _ in range(2)]


def test_check_parameters_needs_no_gpu():
    cpu = torch.device("cpu")
    assert DeviceActor.check_parameters(_actor_tensors(47, 256), 47, 256, cpu) is True
    assert DeviceActor.check_parameters(_actor_tensors(47, 256, head=False), 47, 256, cpu) is False
    DeviceCritic.check_parameters(_critic_tensors(53, 256), 53, 256, cpu)

    def refused(match, fn, *a):
        with pytest.raises(ValueError, match=match):
            fn(*a)

    # shape
    refused("shape", DeviceActor.check_parameters, _actor_tensors(41, 256), 47, 256, cpu)
    refused("shape", DeviceActor.check_parameters, _actor_tensors(47, 128), 47, 256, cpu)
    refused("shape", DeviceCritic.check_parameters, _critic_tensors(47, 256), 53, 256, cpu)
    t = _critic_tensors(53, 256)
    t[1]["q_4_weight"] = torch.zeros((256,))  # [H] instead of [1, H]
    refused("shape", DeviceCritic.check_parameters, t, 53, 256, cpu)
    # dtype
    t = _actor_tensors(47, 256)
    t["mu_weight"] = t["mu_weight"].double()
    refused("float32", DeviceActor.check_parameters, t, 47, 256, cpu)
    t = _critic_tensors(53, 256)
    t[0]["q_0_bias"] = t[0]["q_0_bias"].half()
    refused("float32", DeviceCritic.check_parameters, t, 53, 256, cpu)
    # device: these tensors are on the CPU, the object is said to live on a GPU; numpy arrays are no device tensors at all
    refused("is on cpu", DeviceActor.check_parameters, _actor_tensors(47, 256), 47, 256, torch.device("cuda", 0))
    refused("is on cpu", DeviceCritic.check_parameters, _critic_tensors(53, 256), 53, 256, torch.device("cuda", 0))
    t = _actor_tensors(47, 256)
    t["mu_bias"] = np.zeros(6, np.float32)
    refused("torch tensor", DeviceActor.check_parameters, t, 47, 256, cpu)
    # contiguity
    t = _actor_tensors(47, 256)
    t["latent_pi_2_weight"] = torch.zeros((256, 256)).t()
    refused("contiguous", DeviceActor.check_parameters, t, 47, 256, cpu)
    # keys
    t = _actor_tensors(47, 256)
    del t["latent_pi_0_bias"]
    refused("missing", DeviceActor.check_parameters, t, 47, 256, cpu)
    t = _actor_tensors(47, 256)
    t["value_weight"] = torch.zeros(1)
    refused("unknown", DeviceActor.check_parameters, t, 47, 256, cpu)
    t = _critic_tensors(53, 256)
    del t[0]["q_4_bias"]
    refused("missing", DeviceCritic.check_parameters, t, 53, 256, cpu)
    refused("two Q-networks", DeviceCritic.check_parameters, _critic_tensors(53, 256)[:1], 53, 256, cpu)
    # a lone log_std tensor
    for lone in LOG_STD_ARRAYS:
        t = _actor_tensors(47, 256)
        del t[lone]
        refused("needs both", DeviceActor.check_parameters, t, 47, 256, cpu)
    # a view one float into a larger allocation is fine: only 4-byte alignment is asked for
    t = _actor_tensors(47, 256)
    t["latent_pi_0_weight"] = torch.zeros(47 * 256 + 1)[1:].view(256, 47)
    assert DeviceActor.check_parameters(t, 47, 256, cpu) is True


def test_polyak_is_three_rounded_operations():
    f = np.float32
    rng = np.random.default_rng(5)
    old, src = rng.standard_normal(4096).astype(f), rng.standard_normal(4096).astype(f)
    old[::7], src[::7] = 0.0, 0.0  # padding: +0 in both
    # tau = 1: the source, bit for bit, whatever the old value was (NaN included)
    nan_old = np.full_like(old, np.nan)
    assert np.array_equal(polyak(nan_old, src, 1.0).view(np.uint32), src.view(np.uint32))
    got = polyak(old, src, 0.005)
    assert got.dtype == f
    tau, omt = f(0.005), f(1) - f(0.005)
    # each operation on its own, element by element, in float64 with a rounding after each: float32 x float32 is exact in float64
    a = (old.astype(np.float64) * np.float64(omt)).astype(f)
    b = (np.float64(tau) * src.astype(np.float64)).astype(f)
    want = (a.astype(np.float64) + b.astype(np.float64)).astype(f)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.all(got[::7].view(np.uint32) == 0)  # +0 stays +0, not -0
    # the wrong formula would be noticed: the fused form old + tau (src - old) differs somewhere
    fused = (old + tau * (src - old)).astype(f)
    assert np.any(fused.view(np.uint32) != got.view(np.uint32))
    np.testing.assert_allclose(got, fused, rtol=0, atol=4 * 2.0 ** -24 * 8)  # ... but only by rounding (|values| < 8)
    for bad in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            polyak(old, src, bad)
    with pytest.raises(ValueError):
        polyak(old, src[:-1], 0.5)
