"""The wave-partner catalogue (tests/wave_partner_states.py) is what it says, on the CPU.

test_gpu_wave_partners.py asserts that an env's bits do not depend on the env it shares a wave
with unless one of the two has a leg-leg contact.  That assertion is only sound if the states
outside the leg-leg categories cannot have such a contact, in the oracle or in the f32 kernel,
at any of the substeps run.  Each state goes through the f64 oracle one substep at a time
(O.mj_step(..., nsteps=1) chained SUBSTEPS times, under both contact caps) and must

* be of its category: no contact (air), at least 6 contacts, i.e. more than 32 constraint rows
  (knees), a sphere-box contact (boxes), an active limit row (limit), a leg-leg contact at
  substep 1 (legleg, disjoint; disjoint: two pairs of legs with no leg in common);
* outside legleg / disjoint keep every leg-leg candidate pair at least CLEARANCE = 1e-3 m beyond
  its margin at every substep: 50 x the kernel's per-substep position tolerance (2e-5 m), so a
  kernel inside its tolerance sees no leg-leg contact there either.  This is a condition on the
  inputs; the rows in wave_partner_states.SOURCES were picked to meet it.
"""
import numpy as np
import pytest

import common
import wave_partner_states as W
from oracle import oracle as O
from pupperv3_mjx import _abi


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    path = common.write_model(tmp_path_factory.mktemp("wp"), 10)
    m, _, env = common.env_model_and_config(path)
    jr = env.sys_model.jnt_range
    return m, jr, W.catalogue(m, jr)


def test_catalogue_covers_every_category(world):
    m, _, cat = world
    assert {c for _, c, _ in cat} == set(W.CATEGORIES)
    assert len({name for name, _, _ in cat}) == len(cat)
    assert all(1 <= sum(c == k for _, c, _ in cat) <= 2 for k in W.CATEGORIES)
    assert len(W.legleg_pairs(m)) == 24  # 8 leg spheres, the 4 same-leg pairs excluded
    for _, _, st in cat:
        assert all(np.all(np.isfinite(x)) for x in st)
        assert abs(np.linalg.norm(st[0][3:7]) - 1) < 1e-12


@pytest.mark.parametrize("cap", [0, 16])
def test_states_are_of_their_category(world, cap):
    m, jr, cat = world
    for name, c, st in cat:
        pipes = W.substep_pipes(m, st, ncon_max=cap)
        ncon = [int(p[_abi.P_NCON]) for p in pipes]
        first = pipes[0]
        if c in ("air", "limit"):
            assert ncon == [0] * W.SUBSTEPS, (name, ncon)
        if c in ("stand", "tilt", "low"):
            assert min(ncon) >= 1 and not W.has_box_contact(m, first), (name, ncon)
        if c == "knees":
            assert min(ncon) >= 6, (name, ncon)  # 12 frictionloss rows + 4 per contact > 32
        if c == "boxes":
            assert W.has_box_contact(m, first), name
        if c == "limit":
            assert W.active_limit_rows(m, jr, st) >= 1, name
        if c == "air":
            assert W.active_limit_rows(m, jr, st) == 0, name
        assert W.has_legleg_contact(m, first) == (c in W.LEGLEG), name
    # the two knees-down states differ where the contact cap matters
    nhit = {name: int(W.substep_pipes(m, st, 1, cap)[0][_abi.P_NHIT]) for name, c, st in cat if c == "knees"}
    assert min(nhit.values()) <= 8 < max(nhit.values()), nhit


def test_disjoint_state_couples_two_disjoint_leg_pairs(world):
    m, _, cat = world
    for name, c, st in cat:
        if c != "disjoint":
            continue
        legs = {tuple(sorted(common._leg_of_body(int(m.cgeom_bodyid[g])) for g in ab))
                for ab in W.contact_pairs(m, W.substep_pipes(m, st, 1)[0])
                if all(m.cgeom_bodyid[g] != 0 for g in ab)}
        assert len(legs) >= 2 and not any(all(leg in pr for pr in legs) for leg in range(4)), (name, legs)


@pytest.mark.parametrize("cap", [0, 16])
def test_no_legleg_pair_within_clearance_outside_the_legleg_states(world, cap):
    m, _, cat = world
    worst = {}
    for name, c, st in cat:
        if c in W.LEGLEG:
            continue
        clr = [W.legleg_clearance(m, p) for p in W.substep_pipes(m, st, ncon_max=cap)]
        worst[name] = min(clr)
        assert min(clr) >= W.CLEARANCE, (name, clr)
    print("leg-leg clearance [m]:", {k: round(v, 4) for k, v in worst.items()})


def test_chained_substeps_equal_one_call(world):
    """The per-substep records above describe the run the GPU test makes (one call, nsteps = 5)."""
    m, _, cat = world
    for name, _, st in cat:
        q, v, w = st[0], st[1], st[2]
        for _ in range(W.SUBSTEPS):
            q, v, w, _, _ = O.mj_step(m, q, v, w, st[3], nsteps=1)
        q5, v5, w5, _, _ = O.mj_step(m, *st, nsteps=W.SUBSTEPS)
        for a, b in ((q, q5), (v, v5), (w, w5)):
            np.testing.assert_array_equal(a, b, err_msg=name)


def test_model_without_legleg_pairs(world):
    """The env-level tests' model: the pair list compacted to the plane and box pairs, in order."""
    m, _, cat = world
    m2 = W.without_legleg_pairs(m)
    assert m.npair - m2.npair == len(W.legleg_pairs(m)) and not W.legleg_pairs(m2)
    kept = [(int(m.pair_g1[p]), int(m.pair_g2[p])) for p in range(m.npair)
            if (int(m.pair_g1[p]), int(m.pair_g2[p])) not in W.legleg_pairs(m)]
    assert kept == [(int(m2.pair_g1[p]), int(m2.pair_g2[p])) for p in range(m2.npair)]
    for name, c, st in cat:  # the oracle takes it; only the leg-leg states lose contacts
        a, b = O.mj_step(m, *st, nsteps=1)[3], O.mj_step(m2, *st, nsteps=1)[3]
        assert not W.has_legleg_contact(m2, b)
        if c not in W.LEGLEG:
            np.testing.assert_array_equal(a, b, err_msg=name)
