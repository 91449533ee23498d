"""The characters and arrangements of tests/escalation_cases.py, on the CPU: the facts the GPU tests' table relies on.

The GPU tests (tests/test_gpu_escalation_layouts.py) compare every environment of every arrangement with its character's column of one
reference batch.  That says something about esc_select only if the characters really are in contact when the table says so and the
table really reaches the arms it names: both are asserted here, from the oracle and from the host model alone."""

import numpy as np

import escalation_cases as E


def _span(contact):
    """(first, last) launch with a contact, or None."""
    t = np.flatnonzero(contact)
    return (int(t[0]), int(t[-1])) if len(t) else None


def test_characters_touch_when_the_table_says_so():
    o = E.oracle_run()
    spans = [_span(o["contact"][:, c]) for c in range(E.N_CHARACTERS)]
    print("\nfirst and last launch in contact, per character:", spans)
    print("contacts after the last substep, per launch:\n", o["ncon"])
    # floor: the deeper ones arrive one after the other, rest on the floor with 10 to 14 contacts and are off it once they are driven up
    assert spans[:6] == [(1, E.DOWN), (4, E.DOWN), (8, E.DOWN), (11, E.DOWN), None, None], spans[:6]
    for c in E.FLOOR:
        if spans[c]:
            first, last = spans[c]
            assert o["contact"][first:last + 1, c].all(), c
            assert set(o["ncon"][first:E.DOWN, c].tolist()) <= {10, 14}, (c, o["ncon"][:, c])
    # the plateau: 0..2 rest on the floor in the launch before it, in it and in the next; 3 arrives later
    for c in E.DOWN_AT_T_STAR:
        assert o["contact"][E.T_STAR - 1:E.T_STAR + 2, c].all(), c
    assert spans[3][0] > E.T_STAR
    # folded: one stays in contact, two leave early, five never touch
    assert spans[6:14] == [(0, E.LAUNCHES - 1), (0, 4), (0, 1), None, None, None, None, None], spans[6:14]
    assert o["contact"][:, 6].all() and o["contact"][:5, 7].all() and o["contact"][:2, 8].all()
    # free: no collision pass of any launch saw a penetration at all
    assert (o["pen"][:, list(E.FREE)] == 0.0).all(), o["pen"][:, list(E.FREE)]
    # nobody is truncated or fails its IK: a truncated environment would be stepped differently from the launch after
    assert not o["truncated"].any() and o["ik_success"].all()
    # what the table's counts are made of agrees with the oracle where the oracle decides it
    assert E.ESCALATED_AT_T_STAR[list(E.DOWN_AT_T_STAR)].all() and not E.ESCALATED_AT_T_STAR[list(E.FREE)].any()
    assert (E.ESCALATED_AT_T_STAR | ~o["contact"][E.T_STAR]).all(), "a character in contact is escalated"


def test_characters_are_distinct():
    """No two characters share a start pose: a replica stepped as ANOTHER character's replica shows in the comparison."""
    start, act, grip = E.characters()
    assert len({start[c].tobytes() for c in range(E.N_CHARACTERS)}) == E.N_CHARACTERS
    assert (grip == 1.0).all() and act.shape == (E.LAUNCHES, E.N_CHARACTERS, 7)


def test_host_model():
    rng = np.random.default_rng(0)
    for n in (1, 5, 64, 65, 200):
        mask = rng.uniform(size=n) < 0.4
        words, idx = E.words_of(mask), np.flatnonzero(mask)
        assert [E.rth_set_bit(words, r) for r in range(len(idx) + 2)] == idx.tolist() + [-1, -1]
        picked = [e for row in E.selected(mask) for e in row if e >= 0]
        assert sorted(picked) == idx.tolist() and len(picked) == len(set(picked))
    assert [E.per_of(32, k) for k in (0, 8, 9, 16, 17, 24, 25, 32)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert E.grid_of(1) == 8 and E.grid_of(33) == 16 and E.grid_of(4128) == 1032


def test_table_reaches_every_arm():
    table = E.arrangements()
    arms = {name: E.arms(E.ESCALATED_AT_T_STAR[arr]) for name, (n, arr, count) in table.items()}
    for name, a in arms.items():
        print(f"{name}: n {a['n']}, escalated at the plateau {a['count']}, grid {a['grid']}, per {a['per']}, words {a['words']}")
        assert a["count"] == table[name][2]
    want = {"n1_nobody": (1, 0), "n1_everybody": (1, 1), "n5_two": (5, 2), "n32_8": (32, 8), "n32_9": (32, 9), "n32_16": (32, 16),
            "n32_17": (32, 17), "n32_24": (32, 24), "n32_25": (32, 25), "n32_32": (32, 32), "n33_everybody": (33, 33),
            "n64_last_alone": (64, 1), "n65_word1_alone": (65, 1), "n65_all_but_word1": (65, 64), "n127_alternating": (127, 63),
            "n128_alternating": (128, 64), "n129_alternating": (129, 64), "n4128_sparse": (4128, 50), "n4128_strided": (4128, 1100),
            "n4128_most": (4128, 3210)}
    for name, (n, count) in want.items():
        assert (arms[name]["n"], arms[name]["count"]) == (n, count), name
    # every number of environments per workgroup, and both sides of each threshold at G = 8 and at G = 1032
    assert [arms[f"n32_{k}"]["per"] for k in (8, 9, 16, 17, 24, 25, 32)] == [1, 2, 2, 3, 3, 4, 4]
    assert [arms[k]["per"] for k in ("n4128_sparse", "n4128_strided", "n4128_most")] == [1, 2, 4]
    # single escalated environments on the word boundary and at the end of the batch
    for name, e in (("n64_last_alone", 63), ("n65_word1_alone", 64)):
        n, arr, _ = table[name]
        assert np.flatnonzero(E.ESCALATED_AT_T_STAR[arr]).tolist() == [e] and e == n - 1
        assert arms[name]["last_environment"] and arms[name]["word_boundary"] == (n > 64) and arms[name]["count"] == 1
    assert arms["n65_all_but_word1"]["word_boundary"] and not arms["n65_all_but_word1"]["last_environment"]
    assert all(arms[k]["last_environment"] and arms[k]["word_boundary"] for k in ("n4128_sparse", "n4128_strided", "n4128_most"))
    n, arr, _ = table["n65_all_but_word1"]
    assert np.flatnonzero(~E.ESCALATED_AT_T_STAR[arr]).tolist() == [64]
    # the second pass of the word loop, an escalated environment in word 64, a partly filled last word
    big = [a for a in arms.values() if a["n"] == 4128]
    assert len(big) >= 4 and all(a["second_pass"] and a["escalated_in_word_64"] and a["partial_last_word"] and a["words"] == 65 for a in big)
    n, arr, _ = table["n4128_sparse"]
    down = np.flatnonzero(E.ESCALATED_AT_T_STAR[arr])
    assert {4095, 4096, 4127} <= set(down.tolist()) and (down >= 4096).sum() >= 12
    n, arr, _ = table["n4128_strided"]
    assert (np.flatnonzero(E.ESCALATED_AT_T_STAR[arr]) >= 4096).sum() >= 4
    assert any(not a["partial_last_word"] for a in arms.values())
    # a lean launch with nobody to step, a contact-resolving launch with nobody to step
    assert arms["n32_32"]["lean_steps_nobody"] and arms["n33_everybody"]["lean_steps_nobody"] and arms["n1_everybody"]["lean_steps_nobody"]
    assert arms["n1_nobody"]["resolving_steps_nobody"]
    # at least three arrangements hold folded characters, and every character occurs in each of them
    mixed = [name for name, (n, arr, _) in table.items() if set(E.FOLDED) <= set(arr.tolist())]
    assert len(mixed) >= 3 and all(set(table[m][1].tolist()) == set(range(E.N_CHARACTERS)) for m in mixed), mixed
    assert E.FINE_GRAINED in mixed


def test_every_launch_of_the_plateau_arrangements_is_known_where_the_oracle_decides():
    """In the arrangements made of floor characters 0..2 and free ones the oracle's contacts give a lower bound of the escalated count in
    every launch (a character in contact is escalated), which already crosses the thresholds while the floor characters arrive: the
    layouts are exercised in the launches around the plateau too, not at T_STAR alone."""
    o, table = E.oracle_run(), E.arrangements()
    n, arr, _ = table["n32_25"]
    counts = [int(o["contact"][t][arr].sum()) for t in range(E.LAUNCHES)]
    print("\nn32_25, environments in contact per launch (oracle):", counts)
    assert len({E.per_of(32, c) for c in counts}) >= 3 and counts[E.T_STAR] == 25 and counts[-1] == 0
