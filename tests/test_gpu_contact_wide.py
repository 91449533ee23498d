"""GPU tests of the wide contact solve (csrc/contact_wide.h: the coupled Newton solve and the noslip pass with a lane per contact, taken in
scenes without a free body by an environment with more than 21 contacts) against the oracle, which resolves floor and self contacts with
no bound on its contact list."""

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _oracle():
    from parity_util import MANY_CONTACT_TARGETS, many_contact_oracle_run

    return many_contact_oracle_run(MANY_CONTACT_TARGETS, keep=True)


def _check_many_contact_bars(rep, mode):
    o = rep["oracle"]
    # the bars: 1e-9 on joint positions, 1e-8 on velocities in every launch before the environment's oracle stops reproducing itself
    # (its twin, nudged by 1e-13 rad, parts from it) and before it passes 64 contacts; 100 x the twins' distance in the launch they part in
    assert rep["excess_q"].max() < 1e-9 and rep["excess_v"].max() < 1e-8, rep
    # the evidence, from the oracle's own deterministic counts (MANY_CONTACT_TARGETS: 439, 5 and 436 substeps; 2 environments past 64)
    assert o["wide_held"].sum() >= 400 and (o["wide_held"] > 0).sum() >= 10, o["wide_held"]   # > 21 contacts: the wide solve
    assert o["deep_held"].sum() >= 5, o["deep_held"]                                          # > 48 contacts
    assert o["mixed_held"].sum() >= 400 and ((o["mixed_held"] > 0) & (o["wide_held"] > 0)).sum() >= 1, o["mixed_held"]  # floor + self
    assert o["cap_before_split"].sum() >= 2 and (~o["touched"]).sum() >= 2, o
    # overflow: never where neither the oracle nor its twin passed 64 contacts; always where the oracle passed 64 before its twins parted
    # in joint positions OR in contact counts.  The second set is empty here, and not by choice: the targets that pass 64 do so with the
    # shut fingers' pads pressed face to face, whose contact count is the last bit's several substeps before the positions part (one of the
    # two here: 19 contacts against its twin's 23 at qpos 5e-14 apart, then 65 against 61; the kernel, 1e-13 from both, need not pass 64
    # in that substep).  No draw of tools/make_many_contact_targets.py (3400 targets) passes 64 before its twins' counts part.
    assert not rep["overflow"][o["max_ncon"] <= 64].any(), rep["overflow"]
    assert rep["overflow"][o["cap_first"]].all(), rep["overflow"]
    if mode == 7:  # (escalation: exactly the environments the oracle saw contacts in were resolved; mode 3 resolves everyone, unflagged)
        assert np.array_equal(rep["resolved_ever"], o["touched"]), (rep["resolved_ever"], o["touched"])


@pytest.mark.parametrize("mode", [7, 3], ids=["mode 7", "mode 3"])
def test_many_contacts_match_oracle(mode, monkeypatch):
    """22-75 contacts per environment: hands driven into the floor with the fingers open, arms folded onto themselves, both at once, and
    two that pass the 64 contact slots; environment by environment (mode 7) and the whole batch on the contact-resolving kernel (mode 3)."""
    from parity_util import many_contact_summary, run_many_contact_parity

    monkeypatch.delenv("RCSH_CHECK_SKIP", raising=False)
    rep = run_many_contact_parity(mode=mode, oracle=_oracle())
    print(f"\nmode {mode}\n" + many_contact_summary(rep))
    _check_many_contact_bars(rep, mode)


def test_wide_solve_forced_on_few_contacts(monkeypatch):
    """RCSH_CHECK_SKIP bit 5 (read on every launch, csrc/rcs_hip.hip: make_params) sends every coupled environment of a box-less scene to
    the wide solve, whatever its contact count: the floor, self-contact and many-contact workloads at their own bars with the wide solve's
    math alone, apart from the routing by contact count.  The forced run must differ from the default one in the last bits (the switch took
    effect) and both must hold the oracle's bars."""
    from parity_util import run_floor_contact_parity, run_many_contact_parity, run_self_contact_parity

    runs = {}
    for forced in (False, True):
        if forced:
            monkeypatch.setenv("RCSH_CHECK_SKIP", "32")
        else:
            monkeypatch.delenv("RCSH_CHECK_SKIP", raising=False)
        floor = run_floor_contact_parity(n_envs=8, seed=2)
        assert floor["coupled_substeps"] > 500 and floor["max_ncon"] >= 2 and floor["collisions"] == 8, (forced, floor)
        assert floor["max_abs_qpos"] < 1e-7 and floor["max_abs_qvel"] < 1e-5 and floor["flag_mismatches"] == 0, (forced, floor)
        self7 = run_self_contact_parity(n_envs=24, seed=1, launches=40, mode=7)
        assert self7["max_abs_qpos"] < 1e-9 and self7["max_abs_qvel"] < 1e-8 and self7["overflow"] == 0, (forced, self7)
        assert np.array_equal(self7["resolved_ever"], self7["touched"]), (forced, self7)
        self3 = run_self_contact_parity(n_envs=16, seed=1, launches=30, mode=3)
        assert self3["max_abs_qpos"] < 1e-9 and self3["max_abs_qvel"] < 1e-8 and self3["touched"].sum() >= 2, (forced, self3)
        many = run_many_contact_parity(mode=7, oracle=_oracle())
        _check_many_contact_bars(many, 7)
        runs[forced] = (floor, self7, self3, many)
    monkeypatch.delenv("RCSH_CHECK_SKIP", raising=False)
    (f0, s70, s30, m0), (f1, s71, s31, m1) = runs[False], runs[True]
    assert not np.array_equal(f0["qpos_end"], f1["qpos_end"]), "the floor workload took the same path with bit 5 set"
    assert not np.array_equal(s70["qpos_end"], s71["qpos_end"]), "the self-contact workload (mode 7) took the same path with bit 5 set"
    assert not np.array_equal(s30["qpos_end"], s31["qpos_end"]), "the self-contact workload (mode 3) took the same path with bit 5 set"
    # the many-contact workload: the environments that stay at or below 21 contacts take another path; those above take the same one
    few = (m0["oracle"]["max_ncon"] <= 21) & m0["oracle"]["touched"]
    assert not np.array_equal(m0["kq"][few], m1["kq"][few]), "the few-contact environments took the same path with bit 5 set"
