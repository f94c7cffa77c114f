"""A seeded catalogue of single-env physics states by category, for the wave-partner tests
(test_wave_partner_states.py checks it on the CPU, test_gpu_wave_partners.py runs it on the GPU).

The step kernels put envs 2p and 2p + 1 in one wave ("Wave partners"): an
env's result may depend on its partner only through a leg-leg contact in either of them.  The GPU
test lays every ordered (subject, partner, half) combination of this catalogue out as one wave each
and compares bits, so the catalogue has to span what differs between the two halves of a wave: the
contact count (0 ... the cap), the constraint-row count (at most 32 / more than 32: the row slots),
the collider kinds (plane, box; the cull's near-box mask), limit rows, and the leg-leg
factorisations themselves.

Every state is built from tests/common.py's seeded builders on the 10-box model
(common.write_model(tmp, 10)); SOURCES names the builder arguments and the row taken.  The rows
were chosen so that every category outside LEGLEG keeps each leg-leg candidate pair at least
CLEARANCE beyond its margin over the SUBSTEPS substeps the GPU test runs (test_wave_partner_states
asserts it): the f32 kernel then cannot see a leg-leg contact the f64 oracle does not, and the
only leg-leg contacts in a wave are the ones its LEGLEG states bring.
"""
import numpy as np

import collision_geometry as CG
import common
from oracle import oracle as O
from pupperv3_mjx import _abi

CATEGORIES = ("air", "stand", "tilt", "low", "knees", "boxes", "limit", "legleg", "disjoint")
LEGLEG = ("legleg", "disjoint")  # a leg-leg contact at substep 1: the wave takes the leg-leg factorisation
SUBSTEPS = 5
# 50 x the per-substep position tolerance of the kernel against the oracle (2e-5 m)
CLEARANCE = 1e-3

# (name, category, seed, row) of each state: the builder arguments below and the batch row taken.
# Two knees-down states: 6 contacts (36 rows, just past one row slot) and 10 penetrating pairs (over
# the default cap of 8, which keeps the deepest; 10 contacts under max_contacts=16).
SOURCES = (
    ("air", "air", 1, 0), ("stand", "stand", 1, 0), ("tilt", "tilt", 4, 0), ("low", "low", 1, 0),
    ("knees6", "knees", 11, 0), ("knees10", "knees", 11, 5), ("boxes", "boxes", 13, 0),
    ("limit", "limit", 21, 0), ("legleg", "legleg", 50, 0), ("disjoint", "disjoint", 5, 0),
)
KNEES_ROWS = 16  # rows built of the knees-down batch (its joint noise is drawn for the whole batch)


def _row(states, i):
    return tuple(np.array(x[i], dtype=np.float64) for x in states)


def build(category, model, jnt_range, seed, row):
    """One (qpos[19], qvel[18], qacc_warmstart[18], ctrl[12]) of `category`."""
    if category in ("air", "stand", "tilt", "low"):
        return _row(common.random_physics_states(row + 1, seed=seed, mode=category), row)
    if category == "knees":  # test_gpu_edge.test_contact_cap_overflow_keeps_deepest's knees-down states
        qpos, qvel, qws, ctrl = common.states_on_boxes(model, KNEES_ROWS, seed=seed, z_range=(0.085, 0.10))
        qpos[:, 7:] = (np.array(common.DEFAULT_POSE) + np.tile([0, 0.0, 0.6, 0, 0.0, -0.6], 2)
                       + np.random.RandomState(seed + 1).uniform(-0.1, 0.1, size=(KNEES_ROWS, 12)))
        return _row((qpos, qvel, qws, ctrl), row)
    if category == "boxes":
        return _row(common.states_on_boxes(model, row + 1, seed=seed), row)
    if category == "limit":  # test_gpu_physics.test_joint_limit_rows_parity: hinges past their limits, in the air
        qpos, qvel, qws, ctrl = common.random_physics_states(row + 1, seed=seed, mode="air")
        rs = np.random.RandomState(seed + 1)
        for i in range(row + 1):
            over = rs.uniform(0.02, 0.2, 12)
            hi = (np.arange(12) + i) % 2 == 1
            qpos[i, 7:] = np.where(hi, jnt_range[1:, 1] + over, jnt_range[1:, 0] - over)
        return _row((qpos, qvel * 0.1, qws, ctrl), row)
    if category in LEGLEG:
        kind = "any" if category == "legleg" else "disjoint"
        return _row(common.states_with_self_contact(model, jnt_range, row + 1, seed=seed, kind=kind), row)
    raise KeyError(category)


def catalogue(model, jnt_range, categories=CATEGORIES):
    """[(name, category, (qpos, qvel, qws, ctrl)), ...]: SOURCES' states of `categories`, in order."""
    return [(name, c, build(c, model, jnt_range, seed, row)) for name, c, seed, row in SOURCES if c in categories]


def stack(states):
    """A list of single-env states as batch arrays (qpos[n, 19], qvel, qws, ctrl)."""
    return tuple(np.stack([s[k] for s in states]) for k in range(4))


# ------------------------------------------------------------------ what the oracle says of a state
def legleg_pairs(model):
    """Candidate pairs (cgeom indices) between two robot geoms: all of them join two legs."""
    return [(int(model.pair_g1[p]), int(model.pair_g2[p])) for p in range(model.npair)
            if model.cgeom_bodyid[model.pair_g1[p]] != 0 and model.cgeom_bodyid[model.pair_g2[p]] != 0]


def without_legleg_pairs(model):
    """Copy of the model struct whose candidate-pair list has no pair between two robot geoms
    (the list compacted in order): no leg-leg contact can occur, so no wave ever switches
    factorisation and an env's bits cannot depend on its partner at all."""
    m = type(model).from_buffer_copy(model)
    keep = [p for p in range(model.npair)
            if model.cgeom_bodyid[model.pair_g1[p]] == 0 or model.cgeom_bodyid[model.pair_g2[p]] == 0]
    for k, p in enumerate(keep):
        m.pair_g1[k], m.pair_g2[k] = model.pair_g1[p], model.pair_g2[p]
    for k in range(len(keep), model.npair):
        m.pair_g1[k] = m.pair_g2[k] = 0
    m.npair = len(keep)
    return m


def substep_pipes(model, state, nsteps=SUBSTEPS, ncon_max=0):
    """The f64 oracle's pipeline record of each of `nsteps` chained substeps (each holds the body
    poses the substep's collision pass ran on, and its contacts)."""
    q, v, w, ctrl = state
    pipes = []
    for _ in range(nsteps):
        q, v, w, p, _ = O.mj_step(model, q, v, w, ctrl, nsteps=1, ncon_max=ncon_max)
        pipes.append(p)
    return pipes


def contact_pairs(model, pipe):
    """The record's contacts as (cgeom index, cgeom index) pairs."""
    cg = {int(model.cgeom_id[g]): g for g in range(model.ncgeom)}
    n = int(pipe[_abi.P_NCON])
    g = pipe[_abi.P_CON_GEOM:_abi.P_CON_GEOM + 2 * n].reshape(n, 2).astype(int)
    return [(cg[a], cg[b]) for a, b in g]


def has_legleg_contact(model, pipe):
    return any(model.cgeom_bodyid[a] != 0 and model.cgeom_bodyid[b] != 0 for a, b in contact_pairs(model, pipe))


def has_box_contact(model, pipe):
    return any(model.cgeom_type[b] == _abi.GEOM_BOX for _, b in contact_pairs(model, pipe))


def legleg_clearance(model, pipe):
    """min over the leg-leg candidate pairs of (signed distance - margin): the room before the
    nearest of them would become a contact."""
    return min(CG.pair_distance(model, pipe, a, b) - CG.margin(model, a, b) for a, b in legleg_pairs(model))


def active_limit_rows(model, jnt_range, state):
    """Constraint rows the joint limits add: mj_forward's nefc minus that of a copy whose hinges
    are moved well inside their ranges (no limit row).  Meant for airborne states, where moving
    the hinges changes no contact."""
    q, v, w, ctrl = state
    inside = np.array(q)
    lo, hi = jnt_range[1:, 0], jnt_range[1:, 1]
    m = np.array([model.jnt_margin[1 + j] for j in range(12)])
    inside[7:] = np.clip(inside[7:], lo + m + 0.05, hi - m - 0.05)
    a = O.mj_forward(model, q, v, w, ctrl)
    b = O.mj_forward(model, inside, v, w, ctrl)
    assert a["pipe"][_abi.P_NCON] == 0 and b["pipe"][_abi.P_NCON] == 0
    return a["nefc"] - b["nefc"]
