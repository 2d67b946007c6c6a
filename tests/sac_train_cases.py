"""Shared by tests/test_sac_train_host.py (CPU) and tests/test_sac_train.py (GPU): the schedules a urgym_sac_train call is tested
on, what its validation must refuse, and a plain-Python simulation of the loop the call replaces -- DeviceReplay's cursor arithmetic
around the body of tools/train_sac.py's loop with SACLearner's learning_starts rule.  No GPU, no torch."""
from ur_gym_amd import _abi

TOP = 1 << 63


def schedule(**over):
    base = dict(first_slot=0, filled_steps=0, capacity_steps=4, num_iterations=6, steps_per_iteration=1, updates_per_iteration=2,
                uniform_iterations=0, idle_iterations=0, collect_first_draw=5, update_first_draw=100, first_step=1)
    base.update(over)
    return base


# name -> schedule; every one is accepted
SCHEDULES = {
    "wraps at K = 1": schedule(),
    "fills and wraps inside one iteration's reach (K = 3)": schedule(steps_per_iteration=3, num_iterations=3),
    "K = 5 > C": schedule(steps_per_iteration=5, num_iterations=2),
    "from a non-zero cursor, partly filled": schedule(first_slot=2, filled_steps=1, num_iterations=3, collect_first_draw=1 << 40, first_step=7),
    "U, I = 0, 0": schedule(uniform_iterations=0, idle_iterations=0),
    "U, I = 2, 1": schedule(uniform_iterations=2, idle_iterations=1),
    "U, I = 2, 2": schedule(uniform_iterations=2, idle_iterations=2),
    "U, I = 7, 7 with 6 iterations": schedule(uniform_iterations=7, idle_iterations=7),
    "G = 0": schedule(updates_per_iteration=0, num_iterations=3),
    "K = 0 on a filled ring": schedule(first_slot=1, filled_steps=4, steps_per_iteration=0, updates_per_iteration=3, num_iterations=2),
    "K = 0, one iteration": schedule(first_slot=3, filled_steps=2, steps_per_iteration=0, updates_per_iteration=3, num_iterations=1),
    "the last admissible update_first_draw": schedule(update_first_draw=TOP - 12),
    "collect draws wrap at 2^64": schedule(collect_first_draw=(1 << 64) - 2, num_iterations=4),
}

# name -> schedule; every one is refused (include/urgym.h, urgym_sac_schedule)
REFUSED = {
    "negative K": schedule(steps_per_iteration=-1),
    "negative G": schedule(updates_per_iteration=-1),
    "negative U": schedule(uniform_iterations=-1),
    "negative I": schedule(idle_iterations=-1),
    "no iteration": schedule(num_iterations=0),
    "K and G both 0": schedule(steps_per_iteration=0, updates_per_iteration=0, filled_steps=2),
    "first_slot below 0": schedule(first_slot=-1),
    "first_slot at C": schedule(first_slot=4),
    "filled_steps below 0": schedule(filled_steps=-1),
    "filled_steps above C": schedule(filled_steps=5),
    "an update on an empty ring": schedule(steps_per_iteration=0, filled_steps=0),
    "first_step 0": schedule(first_step=0),
    "one update too many for update_first_draw": schedule(update_first_draw=TOP - 11),
    "update_first_draw above 2^63": schedule(update_first_draw=TOP + 1, updates_per_iteration=0),
    "no capacity": schedule(capacity_steps=0),
}


def simulate_loop(*, capacity_steps, first_slot, filled_steps, num_envs, learning_starts, env_steps, draw, adam_step, iterations,
                  steps_per_iteration, updates_per_iteration, update_first_draw):
    """Today's loop in Python integers.  Returns (collections, updates, end): per collection its first slot, first draw and mode; per
    update the draws, the Adam step, the loss slot, the iteration and the ring view it samples; the learner's and the ring's counters
    afterwards."""
    cursor, filled, C = first_slot, filled_steps, capacity_steps  # DeviceReplay
    collections, updates = [], []
    update_draw = update_first_draw
    for i in range(iterations):
        if steps_per_iteration > 0:
            # SACLearner.collect
            mode = _abi.SAMPLE_UNIFORM if env_steps * num_envs < learning_starts else _abi.SAMPLE_GAUSSIAN
            collections.append(dict(iteration=i, collect_first_slot=cursor, collect_first_draw=draw % (1 << 64), collect_mode=mode))
            # DeviceReplay.collect
            cursor = (cursor + steps_per_iteration) % C
            filled = min(C, filled + steps_per_iteration)
            env_steps += steps_per_iteration
            draw += steps_per_iteration
        if env_steps * num_envs < learning_starts:  # tools/train_sac.py
            continue
        for _ in range(updates_per_iteration):
            # SACLearner._update_on_device
            adam_step += 1
            updates.append(dict(iteration=i, gather_draw=update_draw, policy_draw=update_draw | TOP, adam_step=adam_step, loss_slot=len(updates),
                                oldest_slot=(cursor - filled) % C, filled_steps=filled))
            update_draw += 1
    return collections, updates, dict(cursor=cursor, filled=filled, env_steps=env_steps, draw=draw, adam_step=adam_step)
