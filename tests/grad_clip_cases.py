"""Inputs the gradient-clipping test files share (tests/test_grad_clip_host.py on the CPU, tests/test_grad_clip.py on the GPU).

The groups are gradient tensors in the fixed order of urgym_*_grad_norm: the actor's eight, or the twelve of both Q-networks.  The
hidden widths are the ones at which a 1024-lane reduction can go wrong: 32 x 32 = 1024 elements is exactly one pass of the lanes,
64 x 64 needs four, 256 x 256 sixty-four, and the 6-element biases need less than one.  The values mix magnitudes from 1e-20 to
1e+15 and signs, so that a float32 accumulation, or a float64 one in another order, differs in the last bits; some elements are
float32 subnormals, and one tensor of every group is all zeros."""
import numpy as np

ACTOR_IN = {"ori": 30, "dyn": 47}  # features of the actor per env kind; the critics take six more (the action)
ENV_ID = {"ori": "UR5OriReach-v1", "dyn": "UR5DynReach-v1"}
CASES = (("ori", 32), ("ori", 64), ("ori", 256), ("dyn", 64))  # the smallest env kind at three widths, one other kind
ZERO_TENSOR = 3  # index of the all-zero tensor of a group: b1
ACTOR_KEYS = ("latent_pi_0_weight", "latent_pi_0_bias", "latent_pi_2_weight", "latent_pi_2_bias", "mu_weight", "mu_bias", "log_std_weight", "log_std_bias")
CRITIC_KEYS = ("q_0_weight", "q_0_bias", "q_2_weight", "q_2_bias", "q_4_weight", "q_4_bias")


def actor_shapes(kind, H):
    n = ACTOR_IN[kind]
    return [(H, n), (H,), (H, H), (H,), (6, H), (6,), (6, H), (6,)]


def critic_shapes(kind, H):
    n = ACTOR_IN[kind] + 6
    return 2 * [(H, n), (H,), (H, H), (H,), (1, H), (1,)]


def shapes(which, kind, H):
    return actor_shapes(kind, H) if which == "actor" else critic_shapes(kind, H)


def words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(words(a), words(b))


def same64(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def group(which, kind, H, seed=0):
    """The gradient tensors of one group, float32, in the group's order."""
    rng = np.random.default_rng([seed, H, ACTOR_IN[kind], which == "actor"])
    out = []
    for k, shape in enumerate(shapes(which, kind, H)):
        g = (rng.standard_normal(shape) * np.power(10.0, rng.uniform(-20.0, 15.0, shape))).astype(np.float32)
        flat = g.reshape(-1)
        tiny = rng.integers(0, 9, flat.size) == 0
        flat[tiny] = (rng.integers(-50, 50, int(tiny.sum())) * 1e-41).astype(np.float32)  # float32 subnormals (and a zero or two)
        if k == ZERO_TENSOR:
            flat[:] = 0.0
        out.append(g)
    assert any(((np.abs(g) < np.finfo(np.float32).tiny) & (g != 0)).any() for g in out)
    return out


def moderate_group(which, kind, H, seed=0):
    """Gradients of order 1e-3 .. 1: what a step is tested on (with the wide ones above every stepped value would be +-lr)."""
    rng = np.random.default_rng([seed, H, ACTOR_IN[kind], which == "actor", 7])
    return [(rng.standard_normal(shape) * np.power(10.0, rng.uniform(-3.0, 0.0, shape))).astype(np.float32) for shape in shapes(which, kind, H)]


def as_actor_dict(tensors):
    return dict(zip(ACTOR_KEYS, tensors))


def as_critic_dicts(tensors):
    return [dict(zip(CRITIC_KEYS, tensors[:6])), dict(zip(CRITIC_KEYS, tensors[6:]))]


def with_element(tensors, tensor, index, value):
    """A copy of the group with one flat element replaced (NaN, +inf, -inf)."""
    out = [g.copy() for g in tensors]
    out[tensor].reshape(-1)[index] = value
    return out
