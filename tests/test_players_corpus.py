"""The corpus of the players' step (tests/players_model.py) reaches every arm of host/player.c -- judged on the model alone, from the
states before and after each tick, so that the GPU tests cannot pass by never reaching an arm: the six push-back outcomes of
main.c:212-266, the floor clamp, a step up and a step down between '"' and '#' / '&', a walk through a portal of every rotation
0..3 in each direction and into an unpaired letter, a position outside the grid on each axis, a turn through the sine's general path."""
import numpy as np
import pytest

import players_model as M


@pytest.fixture(scope="module")
def events():
    data, pmap = M.shipped_level()
    hd, hp = M.parse_level(M.HAND_LEVEL)
    per = {}
    per["states"], _ = M.walk_events(data, pmap, M.corpus_states(data), 1 / 60, 8)
    per["edges"], _ = M.walk_events(data, pmap, M.edge_walkers(data, pmap), 1 / 60, 14)
    per["hand"], _ = M.walk_events(hd, hp, M.edge_walkers(hd, hp), 1 / 60, 14)
    per["turners"], _ = M.walk_events(data, pmap, M.turners(), 1e6, 1)
    return per


@pytest.mark.parametrize("what", M.WANTED)
def test_corpus_shows(events, what):
    assert any(what in e for e in events.values()), {k: sorted(v) for k, v in events.items()}


def test_hand_level_has_every_rotation_from_both_ends_and_an_unpaired_letter(events):
    hd, hp = M.parse_level(M.HAND_LEVEL)
    for letter, rot in M.HAND_ROT12.items():
        assert hp[ord(letter) - 65, 4] == rot and hp[ord(letter) - 65, 2] != -1
    assert hp[ord("E") - 65, 0] != -1 and hp[ord("E") - 65, 2] == -1
    want = {"portal %s rot %d" % (w, r) for w in ("1->2", "2->1") for r in range(4)} | {"portal unpaired"}
    assert want <= events["hand"], sorted(events["hand"])


def test_turners_leave_the_position_alone_and_turn():
    """tdiff 1e6 with no move keys: the position stays in the domain, the rows x and z turn by sinf / cosf of +-3e6"""
    data, pmap = M.shipped_level()
    keys, cams, grav, trav = M.turners()
    c, g, t = M.model_step(data, pmap, keys, 1e6, 1, cams, grav, trav)
    assert (c[:, 12] == cams[:, 12]).all() and (c[:, 14] == cams[:, 14]).all() and (c[:, 13] == cams[:, 13]).all()
    assert (c[:, [0, 2, 8, 10]] != cams[:, [0, 2, 8, 10]]).any(axis=1).all()
    assert np.isfinite(c).all() and np.isfinite(g).all()


def test_corpus_is_seeded():
    data, _ = M.shipped_level()
    a, b = M.corpus_states(data), M.corpus_states(data)
    assert all((x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(a, b))
    assert len(a[0]) == 4096
