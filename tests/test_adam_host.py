"""CPU tests (-m "not gpu") of the Adam step that repacks.

  * tests/adam_harness.cpp, a stand-alone host program: the quad map of urgym_pack_map.h names every element of every source tensor
    exactly once (every env kind x hidden width in {32, 160, 256, 288, 512}, actor and critic) -- the property "every parameter is
    stepped exactly once" rests on -- and adam_element of urgym_adam.h, the function the kernels compile, equals evaluation.adam_step
    bit for bit on the GPU tests' input set.  Built a second time with -fsanitize=address,undefined and run as that program.
  * the ctypes mirrors of the new structs, the new symbols, urgym_adam_coefficients against the float64 formulas, and every refusal
    that needs no device.
  * evaluation.adam_step against torch.optim.Adam in float64, with a bound derived from the float32 format (adam_cases.p_bound), and
    its moments against 2^-20 times the same recursions on |g| and g^2.
"""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from adam_cases import HYPER, STEPS, p_bound, same, wide_gradients
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import adam_coefficients, adam_step

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
NEW_SYMBOLS = ("urgym_adam_coefficients", "urgym_actor_adam_step", "urgym_critic_adam_step")
WIDTHS = (32, 160, 256, 288, 512)


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "adam_harness.cpp")
    deps = [src, os.path.join(CSRC, "urgym_adam.h"), os.path.join(CSRC, "urgym_pack_map.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("adam_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("adam_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def check_map_output(run):
    assert run.returncode == 0 and "FAIL" not in run.stdout and not run.stderr, (run.stdout[-2000:], run.stderr[-2000:])
    lines = run.stdout.splitlines()
    assert lines[-1] == "ok 40"
    for n_in in (30, 32, 41, 47):
        for H in WIDTHS:
            # the element counts are the tensors' own: W0, b0, W1, b1 and the heads
            assert any(l.startswith(f"actor in={n_in} H={H} elements={H * n_in + H + H * H + H + 2 * (6 * H + 6)} ") for l in lines), (n_in, H)
            assert any(l.startswith(f"critic in={n_in + 6} H={H} elements={2 * (H * (n_in + 6) + H + H * H + H + H + 1)} ") for l in lines), (n_in, H)


def test_every_element_is_named_by_exactly_one_quad_and_slot(harness):
    check_map_output(subprocess.run([harness], capture_output=True, text=True))


def run_arithmetic(exe, tmp_path, hp, step, p, g, m, v):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<4dqq", hp["lr"], hp["betas"][0], hp["betas"][1], hp["eps"], step, p.size))
        for x in (p, g, m, v):
            f.write(np.ascontiguousarray(x, dtype=np.float32).tobytes())
    run = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (run.stdout, run.stderr[-2000:])
    out = np.fromfile(dst, dtype=np.float32)
    assert out.size == 7 + 3 * p.size
    return out[:7], out[7:7 + p.size], out[7 + p.size:7 + 2 * p.size], out[7 + 2 * p.size:]


def carried_steps(exe, tmp_path, n):
    """The GPU tests' input set through the harness: zeros as moments at step 1, the previous output afterwards."""
    rng = np.random.default_rng(15)
    p, m, v = rng.standard_normal(n).astype(np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    seen_subnormal = seen_underflow = False
    for step in STEPS:
        g = wide_gradients(rng, n)
        gg = g * g
        seen_subnormal |= bool(np.any((gg != 0) & (gg < np.finfo(np.float32).tiny)))
        seen_underflow |= bool(np.any((gg == 0) & (g != 0)))
        coef = adam_coefficients(None, step=step, **HYPER)
        got_coef, got_p, got_m, got_v = run_arithmetic(exe, tmp_path, HYPER, step, p, g, m, v)
        assert same(got_coef, coef), (step, got_coef, coef)  # urgym_adam.h's coefficients are the library's
        p, m, v = adam_step(p, g, m, v, coef)
        assert same(got_p, p) and same(got_m, m) and same(got_v, v), step
        assert np.isfinite(p).all()
    assert seen_subnormal and seen_underflow  # the set does reach what it is meant to reach


def test_shared_arithmetic_equals_adam_step_bitwise(harness, tmp_path):
    carried_steps(harness, tmp_path, 20000)


def test_harness_is_clean_under_address_and_undefined_sanitizers(sanitized_harness, tmp_path):
    check_map_output(subprocess.run([sanitized_harness], capture_output=True, text=True))
    carried_steps(sanitized_harness, tmp_path, 4099)


def test_adam_structs_mirror_the_header():
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()

    def fields(struct_name, types):
        body = hdr[hdr.index(f"typedef struct {struct_name} {{"):hdr.index(f"}} {struct_name};")]
        return re.findall(rf"^\s*({types})\s+(\w+)(\[2\])?;", body, flags=re.M)

    ctype = {"double": C.c_double, "int64_t": C.c_int64, "int32_t": C.c_int32}
    got = fields("urgym_adam_hyper", "double|int64_t|int32_t")
    assert [(n, ctype[t]) for t, n, _ in got] == list(_abi.AdamHyper._fields_) and len(got) == 6
    assert C.sizeof(_abi.AdamHyper) == 48 and _abi.AdamHyper.step.offset == 32 and _abi.AdamHyper.reserved0.offset == 40
    for name, ptr in (("urgym_actor_tensors", r"float\*"), ("urgym_actor_tensors_const", r"const float\*")):
        got = fields(name, ptr)
        assert [n for _, n, _ in got] == list(_abi.ACTOR_DEV_ARRAYS) == [n for n, _ in _abi.ActorTensors._fields_]
    got = fields("urgym_actor_adam", "int32_t|urgym_actor_tensors|urgym_actor_tensors_const")
    assert [n for _, n, _ in got] == ["in_features", "hidden_width", "reserved0"] + list(_abi.ADAM_SETS) == [n for n, _ in _abi.ActorAdam._fields_]
    assert [t for t, _, _ in got[3:]] == ["urgym_actor_tensors", "urgym_actor_tensors_const", "urgym_actor_tensors", "urgym_actor_tensors"]
    got = fields("urgym_critic_adam", "int32_t|urgym_q_network_grad|urgym_q_network_dev")
    assert [n for _, n, _ in got] == [n for n, _ in _abi.CriticAdam._fields_]
    assert [(t, d) for t, _, d in got[3:]] == [("urgym_q_network_grad", "[2]"), ("urgym_q_network_dev", "[2]"), ("urgym_q_network_grad", "[2]"),
                                               ("urgym_q_network_grad", "[2]")]
    # three int32 and then pointers: the compiler pads to 8, and so does ctypes
    assert _abi.ActorAdam.param.offset == 16 and C.sizeof(_abi.ActorAdam) == 16 + 32 * 8
    assert _abi.CriticAdam.param.offset == 16 and C.sizeof(_abi.CriticAdam) == 16 + 48 * 8
    assert _abi.ABI_VERSION == 4 and "#define URGYM_ABI_VERSION 4" in hdr  # added within version 4
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
        assert re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym
    assert lib.urgym_abi_version() == 4
    assert "m' = (b1 * m) + (omb1 * g)" in hdr and "p' = p - (step_size * u)" in hdr  # the arithmetic is stated in the header


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


@pytest.mark.parametrize("lr", (1e-4, 1e-2, 3e-4))
def test_coefficients_are_the_float64_formulas_rounded_once(lr):
    b1, b2, eps = 0.9, 0.999, 1e-8
    for step in (1, 2, 10, 1000, 10 ** 6):
        got = adam_coefficients(None, lr, (b1, b2), eps, step)
        assert got.dtype == np.float32 and got.shape == (7,)
        want = (b1, 1.0 - b1, b2, 1.0 - b2, lr / (1.0 - b1 ** step), np.sqrt(1.0 - b2 ** step), eps)
        for name, g, w in zip(_abi.ADAM_COEFFICIENTS, got, want):
            assert abs(float(g) - w) <= ulp32(w), (step, name, float(g), w)
        # the four that involve no pow are exact roundings
        for i in (0, 1, 2, 3, 6):
            assert got[i] == np.float32(want[i])
    # other betas, beta = 0 included (corr = 1 at every step)
    got = adam_coefficients(None, 1e-3, (0.0, 0.5), 1e-6, 3)
    assert got[0] == 0 and got[1] == 1 and got[4] == np.float32(1e-3) and got[5] == np.float32(np.sqrt(0.875))


def test_refusals_that_need_no_device():
    lib = _native.lib()
    out = (C.c_float * 7)()
    hyper = lambda **over: _abi.AdamHyper(**dict(dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, step=1, reserved0=0), **over))  # noqa: E731
    assert lib.urgym_adam_coefficients(C.byref(hyper()), out) == _abi.OK
    assert lib.urgym_adam_coefficients(C.byref(hyper(lr=0.0)), out) == _abi.OK and out[4] == 0.0  # lr = 0 is a legitimate schedule value
    assert lib.urgym_adam_coefficients(None, out) == _abi.ERR_ARG
    assert lib.urgym_adam_coefficients(C.byref(hyper()), None) == _abi.ERR_ARG
    nan, inf = float("nan"), float("inf")
    bad = [dict(lr=-1e-4), dict(lr=nan), dict(lr=inf), dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=nan), dict(beta2=1.0), dict(beta2=-0.1),
           dict(beta2=nan), dict(eps=0.0), dict(eps=-1e-8), dict(eps=nan), dict(eps=inf), dict(step=0), dict(step=-3), dict(reserved0=1)]
    for over in bad:
        assert lib.urgym_adam_coefficients(C.byref(hyper(**over)), out) == _abi.ERR_ARG, over
        if "reserved0" not in over:  # the Python layer has no way to set it
            with pytest.raises(_native.NativeError):
                adam_coefficients(None, **{**dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, step=1), **_python_form(over)})
    # a NULL handle is refused before anything else is looked at
    hp = hyper()
    assert lib.urgym_actor_adam_step(None, None, None, C.byref(hp), None) == _abi.ERR_ARG
    assert lib.urgym_critic_adam_step(None, None, None, None, C.byref(hp), 0.005, None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    # adam_step refuses what is not the library's coefficients
    z = np.zeros(3, np.float32)
    with pytest.raises(ValueError):
        adam_step(z, z, z, z, np.zeros(7, np.float64))
    with pytest.raises(ValueError):
        adam_step(z, z, z[:2], z, adam_coefficients(None, 1e-4))


def _python_form(over):
    out = {}
    for k, val in over.items():
        if k == "beta1":
            out["betas"] = (val, 0.999)
        elif k == "beta2":
            out["betas"] = (0.9, val)
        else:
            out[k] = val
    return out


# ------------------------------------------------------------------------------------------------ against float64
def cpu_inputs(n, seed):
    """20,000 values: parameters normal; gradients normal times a per-element scale from e^-30 to e^2, every seventh exactly 0."""
    rng = np.random.default_rng(seed)
    p0 = rng.standard_normal(n).astype(np.float32)
    scale = np.exp(rng.uniform(-30.0, 2.0, n))
    grads = []
    for _ in range(5):
        g = (rng.standard_normal(n) * scale).astype(np.float32)
        g[::7] = 0.0
        grads.append(g)
    return p0, grads


@pytest.mark.parametrize("lr", (1e-4, 1e-2))
def test_adam_step_against_torch_adam_in_float64(lr):
    n = 20000
    p0, grads = cpu_inputs(n, 7)
    ref = torch.from_numpy(p0.astype(np.float64)).requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=lr)  # betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad: the defaults
    b1, b2 = 0.9, 0.999
    p, m, v = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    m_mag, v_mag = np.zeros(n), np.zeros(n)  # the same recursions on |g| and g^2 in float64: the scale of the moments' rounding errors
    p0_max = float(np.abs(p0).max())
    for t, g in enumerate(grads, start=1):
        ref.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
        p, m, v = adam_step(p, g, m, v, adam_coefficients(None, lr, (b1, b2), 1e-8, t))
        g64 = g.astype(np.float64)
        m_mag, v_mag = b1 * m_mag + (1 - b1) * np.abs(g64), b2 * v_mag + (1 - b2) * g64 * g64
        state = opt.state[ref]
        err_p = np.abs(p.astype(np.float64) - ref.detach().numpy()).max()
        err_m = np.abs(m.astype(np.float64) - state["exp_avg"].numpy())
        err_v = np.abs(v.astype(np.float64) - state["exp_avg_sq"].numpy())
        bound = p_bound(t, p0_max, lr)
        ratio_m = float((err_m / np.maximum(m_mag, 1e-300)).max()) * 2.0 ** 20
        ratio_v = float((err_v / np.maximum(v_mag, 1e-300)).max()) * 2.0 ** 20
        print(f"lr={lr} step {t}: |p - p64| max {err_p:.3e} of bound {bound:.3e} ({err_p / bound:.2f}); m {ratio_m:.3f}, v {ratio_v:.3f} of 2^-20 x magnitude")
        assert err_p <= bound, (t, err_p, bound)
        assert np.all(err_m <= 2.0 ** -20 * m_mag) and np.all(err_v <= 2.0 ** -20 * v_mag), (t, ratio_m, ratio_v)
    assert np.all(m[::7] == 0) and np.all(v[::7] == 0) and same(p[::7], p0[::7])  # a gradient that is always 0 moves nothing
