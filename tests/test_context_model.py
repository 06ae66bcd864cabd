"""The CPU half of the random call sequences (tests/context_model.py): the model agrees with what the suite already trusts, and
the seed list that tests/test_gpu_context_model.py runs covers the contract -- from the generator and the oracle alone, no GPU."""
import numpy as np
import pytest

import context_model as CM
import handout as H
import hard_scenes as HS


# ---------------------------------------------------------------- the model against what the suite trusts ----

def _walk_model(w, h):
    """a model on handout's level and spheres, and the walk's cameras as inputs"""
    O, path, sph, _ = H.scene(H.LEVEL)
    m = CM.Model(w, h)
    m.apply({"op": "level", "level": H.LEVEL})
    m.apply({"op": "objects", "table": "own"}, {"spheres": sph})
    return m


def test_a_blocking_plane_is_handouts_chain():
    w, h, ks = 96, 64, (0, 1, 2, 3)
    frames = H.chain(H.LEVEL, w, h, ks)
    m = _walk_model(w, h)
    m.apply({"op": "blur", "n": 1})
    for k, (pre, z, post) in zip(ks, frames):
        cam, sec = H.walk(H.LEVEL, k)
        out = m.apply({"op": "frame", "sec": sec}, {"cams": cam[None]})
        H.same(("blocking", k), out["sbuf"], out["zbuf"], post, z)


def test_a_view_slot_is_handouts_chain():
    """slot s of call j is shown the walk's frame j + s, as tests/test_gpu_handout.py test_view_slots shows them"""
    w, h = 96, 64
    m = _walk_model(w, h)
    m.apply({"op": "blur", "n": 0})
    chains = [H.chain(H.LEVEL, w, h, tuple(range(s, s + 3))) for s in range(2)]
    for j in range(3):
        cs = [H.walk(H.LEVEL, j + s) for s in range(2)]
        out = m.apply({"op": "views", "secs": [t for _, t in cs]}, {"cams": np.stack([c for c, _ in cs])})
        for s in range(2):
            pre, z, post = chains[s][j]
            H.same(("views", j, s), out["sbuf"][s], out["zbuf"][s], pre, z)


def test_a_viewport_rectangle_is_a_fresh_context_of_its_size():
    W, Hh = 96, 64
    O = H.scene(H.LEVEL)[0]
    m = _walk_model(W, Hh)
    m.apply({"op": "blur", "n": 1})
    rects = CM.layouts(W, Hh)[2]
    cs = [H.walk(H.LEVEL, i) for i in range(len(rects))]
    out = m.apply({"op": "viewports", "secs": [t for _, t in cs]}, {"cams": np.stack([c for c, _ in cs]), "rects": np.array(rects, np.int32)})
    cover = np.zeros((Hh, W), bool)
    for (x, y, w, h), (cam, sec) in zip(rects, cs):
        sb, z, _ = HS.fresh(O, w, h, cam, sec, True)
        H.same(("viewport", x, y), out["sbuf"][y:y + h, x:x + w], out["zbuf"][y:y + h, x:x + w], sb, z)
        cover[y:y + h, x:x + w] = True
    assert not cover.all() and (out["sbuf"][~cover] == 0).all() and (CM.bits(out["zbuf"])[~cover] == 0).all()


# ---------------------------------------------------------------- the seed list covers the contract ----

_logs = {}


def _log(seed, profile, n_ops):
    """(records, the model's log) of a sequence, through a tracking model, once"""
    if seed not in _logs:
        p = CM.PROFILES[profile]
        ops = CM.generate(seed, n_ops, profile)
        m = CM.Model(p["w"], p["h"], track=True)
        for rec in ops:
            m.apply(rec)
        assert len(m.log) == len(ops)
        _logs[seed] = (ops, m.log)
    return _logs[seed]


def _all_logs():
    return [_log(*s) for s in CM.SEEDS]


def test_the_generator_is_deterministic():
    for seed, profile, n_ops in CM.SEEDS[:3]:
        a, b = CM.generate(seed, n_ops, profile), CM.generate(seed, n_ops, profile)
        assert a == b and len(a) >= n_ops
    assert CM.generate(1, 64, "small") != CM.generate(2, 64, "small")


def test_the_profiles_are_the_issues():
    prof = [p for _, p, _ in CM.SEEDS]
    assert prof.count("small") > len(prof) // 2
    assert prof.count("odd") >= 2 and CM.PROFILES["odd"]["w"] % 4 != 0
    assert 1 <= prof.count("strips") <= 2 and prof.count("one_per_cu") == 1
    h = CM.PROFILES["strips"]["h"]
    assert sorted(CM.strips_of(h, k) for k in (2, 3, 4)) == [2, 3, 3]            # several strips of whole 32-row tiles
    p = CM.PROFILES["one_per_cu"]
    assert H.units_of(p["h"], p["w"]) > 1024 and p["env"] == {"PWN_DBG_BLOCKS_PER_CU": "1"}
    assert len({s for s, _, _ in CM.SEEDS}) == len(CM.SEEDS)


def test_every_ordered_pair_of_families_occurs():
    seen = set()
    for ops, _ in _all_logs():
        fams = [CM.FAMILY.get(r["op"]) for r in ops]
        seen |= {(a, b) for a, b in zip(fams, fams[1:]) if a and b}
    missing = [a + b for a in CM.FAMILIES for b in CM.FAMILIES if (a, b) not in seen]
    assert not missing, missing


@pytest.mark.parametrize("seed,profile,n_ops", CM.SEEDS)
def test_depth_persistence_is_visible_in_every_plane_owning_family(seed, profile, n_ops):
    """in every sequence, each of the blocking call, the view slots, the viewports and the frame slots has a frame whose primary
    rays run out of steps at pixels where the plane held a non-zero depth that a different camera left"""
    _, log = _log(seed, profile, n_ops)
    seen = set()
    for e in log:
        seen |= set(e["persist"])
    assert seen == set(CM.PLANE_OWNERS), (seed, sorted(seen))


def test_every_family_runs_in_form_2_and_right_behind_a_switch():
    in2, after = set(), set()
    for _, log in _all_logs():
        for e in log:
            if e["ran"] and e["fam"] in CM.LAUNCHING:
                if e["form2"]:
                    in2.add(e["fam"])
                if e["after_switch"]:
                    after.add((e["fam"], e["after_switch"]))
    assert in2 == set(CM.LAUNCHING), sorted(in2)
    # (both directions, each family)
    assert after == {(f, d) for f in CM.LAUNCHING for d in ("to2", "from2")}, sorted(after)


def test_every_blurred_family_runs_under_0_to_3_passes():
    seen = {(e["fam"], e["blur"]) for _, log in _all_logs() for e in log if e["ran"] and e["fam"] in CM.BLURRED}
    assert seen >= {(f, p) for f in CM.BLURRED for p in range(4)}, sorted(seen)


def test_every_modelled_error_is_expected():
    logs = [e for _, log in _all_logs() for e in log]
    # PWN_EINVAL for w % 4 != 0 with blur on, in every family that blurs (the strip forms' blur among them)
    refused = {e["fam"] for e in logs if e["err"] == CM.EINVAL and e["blur"] > 0 and e["fam"] != "-"}
    assert refused >= set(CM.BLURRED), sorted(refused)
    assert any(e["op"] == "rows" and e["err"] == CM.EINVAL for e in logs)
    assert any(e.get("slot_busy") for e in logs) and any(e.get("overlap_busy") for e in logs)
    assert {e["fam"] for e in logs if e["err"] == CM.ENOLEVEL} >= set(CM.LAUNCHING), sorted({e["fam"] for e in logs if e["err"] == CM.ENOLEVEL})
    assert any(e["op"] == "prepare" and e["err"] == CM.EINVAL for e in logs)


def test_the_odd_width_goes_on_unharmed_after_a_refusal():
    """at w % 4 != 0 every blurred call with passes > 0 is refused, and the same families run again afterwards"""
    for (seed, profile, n_ops) in CM.SEEDS:
        if profile != "odd":
            continue
        _, log = _log(seed, profile, n_ops)
        for e in log:
            if e["fam"] in CM.BLURRED and e["blur"] > 0 and e["op"] not in ("config", "wait"):
                assert e["err"] in (CM.EINVAL, CM.EBUSY), e
        first = min(i for i, e in enumerate(log) if e["err"] == CM.EINVAL)
        assert {e["fam"] for e in log[first:] if e["ran"]} >= set(CM.LAUNCHING), seed


def test_outside_the_viewports_is_checked_behind_a_call_that_covered_it():
    assert any(e.get("vp_outside_after_cover") for _, log in _all_logs() for e in log)
    for _, log in _all_logs():
        assert any(e["op"] == "config" and e["err"] == CM.OK for e in log)
