"""The corpus of the pwn_trace_reach tests (tests/reach_chain.py) reaches every arm of the definition -- the model alone, on the oracle's
event chains, no GPU: FREE in a plain room cell, a fog cell and a ramp cell of each kind, in a two-high room after a y shift, behind
1, 2 and >= 3 portals with every rotation from both ends, in the step right behind a crossing; wall and sphere within reach; a
sphere candidate beyond reach with the wall further still; a wall at cdist > reach in the same step; PWN_HIT_NONE; reach 0, negative,
NaN and +inf.  And the model leaves out at most 1 % of any batch."""
import numpy as np
import pytest

import hit_chain as HC
import reach_chain as RC


@pytest.fixture(scope="module")
def seen(oracle_lib):
    """what the corpus reaches: a set of tags, and per batch the share the model left out"""
    tags, left = set(), []
    for pi, part in enumerate(RC.corpus(oracle_lib)):
        n = len(part.rays)
        for bi, reach in enumerate(RC.reaches(pi, part)):
            w = RC.model(part.chains, reach)
            left.append((part.name, bi, int(w.left_out.sum()), n))
            for i in np.flatnonzero(~w.left_out):
                c, arm, r = part.chains[i], str(w.arm[i]), reach[i]
                tags.add(arm)
                with np.errstate(invalid="ignore"):
                    if bi == 8 and (c.cdist[1:] == r).any() and not (c.cdist[1:] > r).any() and not arm.startswith("free"):
                        tags.add("exact_cdist_walks_on")
                    if bi == 8 and c.ev != HC.NONE and c.dist == r and not arm.startswith("free"):
                        tags.add("exact_D_is_within")
                rtag = "nan" if np.isnan(r) else "inf" if np.isinf(r) else "neg" if r < 0 else "zero" if r == 0 else "pos"
                tags.add("reach_" + rtag + ("_free" if arm.startswith("free") else "_hit"))
                if not arm.startswith("free"):
                    # (+inf and NaN: the record is hit_chain's own, whatever it is)
                    if rtag in ("inf", "nan"):
                        assert w.want[i] == c.rec
                    continue
                k = int(w.steps[i]) - 1
                ch = chr(c.ch[k])
                if "A" <= ch <= "Z":
                    assert r < 0 and k == 0, "a portal step is never the reach step; under a negative reach the first step stops the walk"
                    tags.add("free_neg_in_front_of_crossing")
                    continue
                tags.add("free_in_" + ch)
                p = int(w.want["portals"][i])
                tags.add("free_behind_%s_portals" % (p if p < 3 else "3+"))
                for letter, end in c.crossings[:p]:
                    tags.add("free_behind_%s%d" % (letter, end))
                if k > 0 and "A" <= chr(c.ch[k - 1]) <= "Z":
                    tags.add("free_right_behind_crossing")
                before = set(chr(v) for v in c.ch[:k])
                if ch in "#&" and '"' in before:
                    tags.add("free_two_high_after_shift_up")
                if ch == '"' and before & set("#&"):
                    tags.add("free_low_after_shift_down")
                if r == 0 and k == 0:
                    assert (w.want["x"][i], w.want["y"][i], w.want["z"][i]) == tuple(c.pos[0]), "reach 0: FREE at the set-up's pos_0"
    return tags, left


def test_model_leaves_out_at_most_one_percent(seen):
    for name, bi, out, n in seen[1]:
        assert out * 100 <= n, (name, bi, out, n)


WANTED = (["free", "wall", "sphere", "free_sphere_beyond", "free_wall_same_step", "none"]
          + ["free_in_" + c for c in ';$><,^#&"']
          + ["free_two_high_after_shift_up", "free_low_after_shift_down", "free_right_behind_crossing"]
          + ["free_behind_%s_portals" % p for p in (0, 1, 2, "3+")]
          + ["free_behind_%s%d" % (letter, end) for letter in "ABCD" for end in (0, 1)]
          + ["reach_zero_free", "reach_neg_free", "reach_nan_hit", "reach_inf_hit", "reach_pos_free", "reach_pos_hit", "free_neg_in_front_of_crossing",
             "exact_cdist_walks_on", "exact_D_is_within"])


@pytest.mark.parametrize("tag", WANTED)
def test_corpus_reaches(seen, tag):
    assert tag in seen[0], sorted(seen[0])


def test_portal_rotations_are_all_four(oracle_lib):
    """the hand-made level's pairs A, B, C, D turn by 0, 2, 3 and 1 quarter turns (tests/players_model.py's level)"""
    O = oracle_lib.Oracle()
    O.load_level_text(RC.HAND_LEVEL)
    _, pmap, _ = O.get_level()
    assert [int(pmap[i][4]) & 3 for i in range(4)] == [0, 2, 3, 1]


def test_records_within_reach_are_hit_chains(oracle_lib):
    """every ray whose chain shows D <= reach comes out as hit_chain's own record; a FREE record's dist is the reach, bit for bit"""
    for pi, part in enumerate(RC.corpus(oracle_lib)):
        for reach in RC.reaches(pi, part):
            w = RC.model(part.chains, reach)
            for i, c in enumerate(part.chains):
                if w.left_out[i]:
                    continue
                with np.errstate(invalid="ignore"):
                    within = c.ev != HC.NONE and not (c.dist > reach[i]) and not (c.cdist[1:] > reach[i]).any()
                if within:
                    assert w.want[i] == c.rec and w.want["kind"][i] in (HC.WALL, HC.SPHERE)
                if w.want["kind"][i] == RC.FREE:
                    assert np.float32(w.want["dist"][i]).view(np.uint32) == np.float32(reach[i]).view(np.uint32)
                    assert w.want["face"][i] == -1 and w.want["object"][i] == -1
