"""Batch layouts for per-environment escalation (csrc/sim_kernels.h: esc_select, esc_finish; csrc/rcs_hip.hip: launch_run), built from
the oracle alone.

With the robot's contacts resolved environment by environment a step is a lean launch over the environments that are not escalated
and a contact-resolving launch over those that are.  Which workgroup of the contact-resolving launch steps which environment is
decided by esc_select, which ranks the bits of the escalation words: a wrong rank steps an environment twice, not at all, or from a
neighbour's slot, and crashes nothing.  The property the GPU tests (tests/test_gpu_escalation_layouts.py) hold it to: an
environment's trajectory depends on its own inputs only, bit for bit -- not on its index, the batch size or who else is escalated.

CHARACTERS: 16 scripted environments of the headline configuration (fr3_empty_world, JOINTS relative to last_step, asynchronous, 17
substeps a launch, the fused env step, gripper commanded open throughout -- shut fingers pressed together are the one regime in which
the oracle does not reproduce itself).  Each is a hard-set start pose and an action per launch:
  * floor  (0..5)   home with q[1] = 0.8 + 0.03 i, q[3] = -0.8 for i = 15, 12, 9, 6, 3, 0; joint 2 driven +5 degrees a launch for
                    DOWN launches, then -5 degrees for UP launches.  The deeper ones meet the floor one after the other, rest on it and
                    come off it again; i = 3 and i = 0 never reach it;
  * folded (6..13)  eight poses of parity_util.run_self_contact_parity's distribution (seed 1, FOLDED_ROWS), zero action: one touches
                    itself from the first launch on, two do so in the first launch and are clear again a few launches later --
                    escalation that begins at once and ends early --, five never touch;
  * free   (14, 15) home with a small offset, random moves of +-2 degrees: never anywhere near a contact.

ARRANGEMENTS: a name, a batch size n and n character indices.  Every replica of a character gets the character's script, so every
environment of every arrangement has to equal the character's column of the one reference batch that holds each character once -- and
that batch is held to the oracle.  At the plateau launch T_STAR the floor characters 0..2 rest on the floor (escalated) and the free
ones are not escalated, so an arrangement made of those two kinds has an exact escalated count there, chosen to sit on either side of
every threshold of esc_select.

The host model at the end (`per_of`, `rth_set_bit`, `arms`) restates which arm of esc_select a layout reaches.  It documents the
table and is its precondition (tests/test_escalation_cases_cpu.py); nothing is checked against it on the GPU.
"""

from __future__ import annotations

import functools

import numpy as np

SUBSTEPS = 17               # an asynchronous env step at 30 Hz
DOWN, UP = 13, 8            # launches the floor characters are driven down / up again
LAUNCHES = DOWN + UP
T_STAR = 10                 # the plateau launch: floor characters 0..2 rest on the floor, 3 has not arrived
STEP = float(np.deg2rad(5))
OPEN = 0.04                 # finger slides of the open gripper

FLOOR_DEPTHS = (15, 12, 9, 6, 3, 0)
FLOOR = tuple(range(0, 6))
FOLDED = tuple(range(6, 14))
FREE = (14, 15)
N_CHARACTERS = 16
# Rows of the folded distribution's 24 draws.  Hard-set and left alone, on the oracle: row 0 touches itself in launch 0 and stays in
# contact (14 contacts), row 11 is clear again from launch 5 on, row 17 from launch 2 on; no other row of the 24 but row 13 (as row 0)
# touches at all, and rows 1 .. 5 stand for those.
FOLDED_ROWS = (0, 11, 17, 1, 2, 3, 4, 5)
DOWN_AT_T_STAR = (0, 1, 2)  # the floor characters an exact count is made of
KIND = {**{c: "floor" for c in FLOOR}, **{c: "folded" for c in FOLDED}, **{c: "free" for c in FREE}}

# Whether the character is on the contact-resolving launch after launch T_STAR (the `now` bit).  For the floor characters 0..2 (in
# contact: tests/test_escalation_cases_cpu.py) and the free ones it follows from the oracle; for the others -- near a contact, where the
# lean launch's certificate decides -- it is what the reference batch shows, and tests/test_gpu_escalation_layouts.py asserts it there.
ESCALATED_AT_T_STAR = np.array([1, 1, 1, 0, 0, 0,   1, 0, 0, 0, 0, 0, 0, 0,   0, 0], dtype=bool)


def _home():
    from rcs_env_oracle import FR3_Q_HOME

    return np.asarray(FR3_Q_HOME, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def characters():
    """(start [16, 9] -- arm joints and finger slides --, actions [LAUNCHES, 16, 7], gripper [LAUNCHES, 16] f32)."""
    home = _home()
    start = np.tile(np.concatenate([home, [OPEN, OPEN]]), (N_CHARACTERS, 1))
    act = np.zeros((LAUNCHES, N_CHARACTERS, 7))
    for c, i in zip(FLOOR, FLOOR_DEPTHS):
        start[c, 1], start[c, 3] = 0.8 + 0.03 * i, -0.8
        act[:DOWN, c, 1], act[DOWN:, c, 1] = STEP, -STEP
    # (parity_util.run_self_contact_parity draws 24 rows per joint from one generator: the same calls, FOLDED_ROWS of them)
    rng = np.random.default_rng(1)
    for j, (lo, hi) in ((0, (-1, 1)), (1, (-1.78, 0.2)), (3, (-3.04, -2.6)), (4, (-0.5, 0.5)), (5, (0.55, 1.6))):
        start[list(FOLDED), j] = rng.uniform(lo, hi, 24)[list(FOLDED_ROWS)]
    for k, c in enumerate(FREE):
        start[c, :7] = home + 0.05 * (k + 1) * np.array([1, -1, 1, -1, 1, -1, 1.0])
        act[:, c, :] = np.random.default_rng(100 + k).uniform(-0.4 * STEP, 0.4 * STEP, (LAUNCHES, 7))
    start.setflags(write=False)
    act.setflags(write=False)
    grip = np.ones((LAUNCHES, N_CHARACTERS), dtype=np.float32)
    grip.setflags(write=False)
    return start, act, grip


def place_oracle(oe, start9):
    """An oracle environment at a character's start pose: what set_joints_hard plus the qpos write do to an environment of the kernel's."""
    oe.reset()
    oe.sim.set_joints_hard(start9[:7])
    for k in range(7, 9):
        oe.sim.s.d.qpos[k] = float(start9[k])


@functools.lru_cache(maxsize=None)
def oracle_run():
    """Every character on the CPU oracle (floor and self contacts resolved), once: per launch the state, the observation, the flags and the
    deepest penetration any collision pass of the launch saw."""
    from parity_util import make_oracle_envs

    start, act, grip = characters()
    oenvs = make_oracle_envs(N_CHARACTERS, True)
    assert oenvs[0].sim.model.resolve_contacts == 3
    for c, oe in enumerate(oenvs):
        place_oracle(oe, start[c])
    n = N_CHARACTERS
    out = {"pen": np.zeros((LAUNCHES, n)), "ncon": np.zeros((LAUNCHES, n), dtype=int), "qpos": np.zeros((LAUNCHES, n, 9)),
           "qvel": np.zeros((LAUNCHES, n, 9)), "joints": np.zeros((LAUNCHES, n, 7)), "tquat": np.zeros((LAUNCHES, n, 7)),
           "gripper": np.zeros((LAUNCHES, n)), "collision": np.zeros((LAUNCHES, n), dtype=bool), "ik_success": np.zeros((LAUNCHES, n), dtype=bool),
           "truncated": np.zeros((LAUNCHES, n), dtype=bool)}
    for t in range(LAUNCHES):
        for c, oe in enumerate(oenvs):
            oe.sim.s.d.pen_seen = 0.0
            oo, _, _, trunc, oi = oe.step({"joints": act[t, c], "gripper": grip[t, c]})
            out["pen"][t, c], out["ncon"][t, c] = float(oe.sim.s.d.pen_seen), int(oe.sim.s.d.ncon)
            out["qpos"][t, c], out["qvel"][t, c] = np.asarray(oe.sim.qpos)[:9], np.asarray(oe.sim.qvel)[:9]
            out["joints"][t, c], out["tquat"][t, c], out["gripper"][t, c] = oo["joints"], oo["tquat"], float(oo["gripper"])
            out["collision"][t, c], out["ik_success"][t, c], out["truncated"][t, c] = bool(oi["collision"]), bool(oi["ik_success"]), bool(trunc)
    out["contact"] = out["pen"] > 1e-9  # (the threshold parity_util.run_headline_resolved_parity counts a contact by)
    for a in out.values():
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------------------- arrangements
def _two_kinds(n, down):
    """n environments: the positions in `down` take the floor characters that rest on the floor at T_STAR, in turn; the others the free ones."""
    down = np.asarray(sorted(int(e) for e in down), dtype=int)
    assert len(set(down.tolist())) == len(down) and (len(down) == 0 or (0 <= down[0] and down[-1] < n))
    arr = np.asarray(FREE)[np.arange(n) % len(FREE)]
    arr[down] = np.asarray(DOWN_AT_T_STAR)[np.arange(len(down)) % len(DOWN_AT_T_STAR)]
    return arr


def _strided(n, count, stride):
    """`count` distinct positions of [0, n): multiples of a stride that is coprime to n, wrapped."""
    assert np.gcd(n, stride) == 1 and count <= n
    return (np.arange(count) * stride + stride // 2) % n


def _sparse_4128():
    down = [3, 64, 700, 1023, 1024, 2047, 2048, 2049, 3000, 4000, 4032, 4094, 4095, 4096, 4097, 4100, 4103, 4110, 4111, 4112, 4119, 4120, 4125, 4126, 4127]
    down += list(range(130, 3900, 157))  # 25 more, below word 64
    return down


@functools.lru_cache(maxsize=None)
def arrangements():
    """name -> (n, character index per environment, the escalated count the table names for T_STAR)."""
    t = {}

    def add(name, n, arr):
        arr = np.asarray(arr, dtype=int)
        assert arr.shape == (n,) and arr.min() >= 0 and arr.max() < N_CHARACTERS
        arr.setflags(write=False)
        t[name] = (n, arr, int(ESCALATED_AT_T_STAR[arr].sum()))

    add("n1_nobody", 1, _two_kinds(1, []))
    add("n1_everybody", 1, _two_kinds(1, [0]))
    add("n5_two", 5, _two_kinds(5, [1, 4]))
    for k in (8, 9, 16, 17, 24, 25, 32):  # G = 8 workgroups: 1 -> 2, 2 -> 3, 3 -> 4 environments each; 32: the lean launch steps nobody
        add(f"n32_{k}", 32, _two_kinds(32, _strided(32, k, 5)))
    add("n33_everybody", 33, _two_kinds(33, range(33)))
    add("n64_last_alone", 64, _two_kinds(64, [63]))
    add("n65_word1_alone", 65, _two_kinds(65, [64]))
    add("n65_all_but_word1", 65, _two_kinds(65, range(64)))
    for n in (127, 128, 129):
        add(f"n{n}_alternating", n, _two_kinds(n, range(1, n, 2)))
    # 65 words, the last with 32 valid bits; G = 1032 workgroups
    add("n4128_sparse", 4128, _two_kinds(4128, _sparse_4128()))
    add("n4128_strided", 4128, _two_kinds(4128, _strided(4128, 1100, 5)))  # (wraps: 5 k reaches 4096 .. 4127 before it does)
    add("n4128_most", 4128, _two_kinds(4128, [e for e in range(4128) if e % 9 not in (0, 4)]))
    # every character, folded ones included: the merge and the leave bits change in the launches in which the floor characters arrive
    add("n37_mixed", 37, (np.arange(37) * 7 + 2) % N_CHARACTERS)
    add("n70_mixed", 70, (np.arange(70) * 3 + 1) % N_CHARACTERS)
    add("n130_mixed", 130, (np.arange(130) * 11 + 5) % N_CHARACTERS)
    add("n4128_mixed", 4128, (np.arange(4128) * 13 + (np.arange(4128) // 64)) % N_CHARACTERS)
    return t


FINE_GRAINED = "n70_mixed"  # the arrangement that also runs through Sim.step / set_joint_position and through step_until_convergence


# --------------------------------------------------------------------------------------------------------------------- host model
def words_of(mask):
    """[n] bool -> the escalation words, python ints, bit e % 64 of word e // 64."""
    mask = np.asarray(mask, dtype=bool)
    return [sum(1 << b for b in np.flatnonzero(mask[w:w + 64]).tolist()) for w in range(0, len(mask), 64)]


def rth_set_bit(words, r):
    """The index of the r-th set bit (from 0) of a list of 64-bit words; -1: there are not that many."""
    for w, x in enumerate(words):
        c = bin(x).count("1")
        if r < c:
            for _ in range(r):
                x &= x - 1
            return 64 * w + (x & -x).bit_length() - 1
        r -= c
    return -1


def grid_of(n):
    """Workgroups of a launch over n environments: 8 for every 32 of them (launch_run)."""
    return 8 * ((n + 31) // 32)


def per_of(n, count):
    """Environments a workgroup of the contact-resolving launch takes: as few as the launch's workgroups allow."""
    g = grid_of(n)
    return 1 if count <= g else 2 if count <= 2 * g else 3 if count <= 3 * g else 4


def arms(mask):
    """Which arms of esc_select / the two launches a batch with these escalation bits reaches."""
    mask = np.asarray(mask, dtype=bool)
    n, count = len(mask), int(mask.sum())
    nw = (n + 63) // 64
    return {"n": n, "count": count, "grid": grid_of(n), "per": per_of(n, count), "words": nw, "partial_last_word": n % 64 != 0,
            "second_pass": nw > 64, "escalated_in_word_64": bool(mask[4096:].any()), "lean_steps_nobody": count == n,
            "resolving_steps_nobody": count == 0, "last_environment": bool(mask[-1]), "word_boundary": bool(n > 64 and (mask[63] or mask[64]))}


def selected(mask):
    """The environment every (workgroup slot, team) of the contact-resolving launch stands for under the host model: slot r takes the
    environments of rank r per .. r per + per - 1 on its first teams.  Each escalated environment appears exactly once."""
    words, per = words_of(mask), per_of(len(mask), int(np.sum(mask)))
    return [[rth_set_bit(words, r * per + k) if k < per else -1 for k in range(4)] for r in range(grid_of(len(mask)))]
