"""The actor's parameter gradients above one split of 1024 rows (urgym_actor_backward.hip: stage 2 once per split into the workspace,
stage 3 adds the splits in float64): 2049 rows (three splits, the last of one row), 3072, 4513 (five splits and a partial last row
group), and 64,513 and 65,536 rows (64 splits, the cap), on the exact network of tests/test_actor_backward.py in the HEADS form, where
float64 is the bitwise reference.  Each case asserts its own bound on the largest sum of absolute terms (below 2^24 units); dense
upstreams at the cap and H = 256 would pass it, so that case has one nonzero component per row.  The last row of every batch has a
nonzero upstream and live neurons, so a dropped tail shows.
"""
import functools

import numpy as np
import pytest

from test_actor_backward import KEYS, SPLIT, _dev, _env, _rows, assert_exact, bits_equal, edge_network, exact_upstream, forward_f64, gradients_f64
from test_actor_widths import exact_inputs
from ur_gym_amd import _abi
from ur_gym_amd.evaluation import DeviceActor

CAP = _abi.ACTOR_GRADIENTS_MAX_COUNT
MANY_COUNTS = (2 * SPLIT + 1, 3 * SPLIT, 4 * SPLIT + 417)
CAP_COUNTS = (63 * SPLIT + 1, CAP)
MANY_CASES = [(kind, H) for kind in ("dyn", "ori") for H in (32, 160, 256)]  # the HT = 4 instance, HT = 8 padded, HT = 8 full
CAP_CASES = [(H, n) for H in (32, 256) for n in CAP_COUNTS]


@functools.lru_cache(maxsize=4)
def case(kind, H, n, dense=True):
    x = exact_inputs(kind, n)
    net = edge_network(kind, H, x)
    d_mu, d_ls = exact_upstream(net, x, dense=dense)
    ref, worst = assert_exact(net, x, d_mu, d_ls)
    # the last row: a nonzero upstream that reaches live neurons of both layers
    z1, z2, _, _ = forward_f64(net, x[-1:])
    tail = gradients_f64(net, x[-1:], d_mu[-1:], d_ls[-1:])
    assert d_mu[-1].any() and (z1 > 0).any() and (z2 > 0).any() and all(tail[k].any() for k in KEYS[:6]), (kind, H, n)
    return dict(net=net, x=x, d_mu=d_mu, d_ls=d_ls, ref=ref, worst=worst)


def _add(parts):
    return {k: sum(p[k] for p in parts) for k in KEYS}


def _differing(a, b):
    return [k for k in KEYS if not np.array_equal(a[k], b[k])]


@pytest.mark.parametrize("H,n", [(H, n) for H in (32, 256) for n in MANY_COUNTS] + [(32, n) for n in CAP_COUNTS])
def test_split_mistakes_would_show(H, n):
    """The float64 gradients per split of 1024 rows add up to the whole (exactly: every term is a multiple of one unit), and three
    wrong ways of adding them differ from it in all eight tensors."""
    c = case("dyn", H, n)
    net, x, d_mu, d_ls, whole = c["net"], c["x"], c["d_mu"], c["d_ls"], c["ref"]
    print(f"dyn H={H} count={n}: largest sum of absolute terms {c['worst']:.4g} units (2^24 = {2.0 ** 24:.4g})")
    S = (n + SPLIT - 1) // SPLIT
    bounds = [(s * SPLIT, min(n, (s + 1) * SPLIT)) for s in range(S)]
    assert S >= 3 and bounds[-1][1] == n
    part = [gradients_f64(net, x[a:b], d_mu[a:b], d_ls[a:b]) for a, b in bounds]
    assert _differing(_add(part), whole) == []
    wrong = {"last split dropped": _add(part[:-1]), "split s >= 2 from the rows of split s - 1": _add(part[:2] + part[1:S - 1])}
    if n % 32:
        a = n // 32 * 32
        tail = gradients_f64(net, x[a:], d_mu[a:], d_ls[a:])
        wrong["last partial row group dropped"] = {k: whole[k] - tail[k] for k in KEYS}
    else:
        assert n in (3 * SPLIT, CAP)
    for label, bad in wrong.items():
        differs = _differing(bad, whole)
        print(f"dyn H={H} count={n} '{label}': differs in {len(differs)} of {len(KEYS)} tensors")
        assert differs == list(KEYS), (H, n, label, differs)


def _check(env, kind, H, n, dense=True):
    import torch

    c = case(kind, H, n, dense)
    print(f"{kind} H={H} count={n} {'dense' if dense else 'sparse'}: largest sum of absolute terms {c['worst']:.4g} units (2^24 = {2.0 ** 24:.4g})")
    actor = DeviceActor(c["net"], env)
    got = env.actor_parameter_gradients(actor, sample=dict(mode="mean"), rows=_rows(kind, c["x"]), d_mu=_dev(c["d_mu"]), d_log_std=_dev(c["d_ls"]))
    torch.cuda.synchronize()
    for key in KEYS:
        assert bits_equal(got["grads"][key].cpu().numpy(), c["ref"][key]), (kind, H, n, key)
    actor.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,H", MANY_CASES, ids=[f"{k}-{H}" for k, H in MANY_CASES])
def test_exact_network_many_splits_on_the_device(kind, H):
    env = _env(kind, 8)
    for n in MANY_COUNTS:
        _check(env, kind, H, n)
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H,n", CAP_CASES, ids=[f"dyn-{H}-{n}" for H, n in CAP_CASES])
def test_exact_network_at_the_cap_on_the_device(H, n):
    env = _env("dyn", 8)
    _check(env, "dyn", H, n, dense=H == 32)
    env.close()
