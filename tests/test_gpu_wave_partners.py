"""An env's result does not depend on the env it shares a wave with ("Wave
partners"), at the bit level.

The step kernels put envs 2p and 2p + 1 in one 64-lane wave.  The contract: an env's trajectory is
a function of its own inputs; its partner may change it in exactly one way -- a leg-leg contact in
either env switches both to the leg-leg Newton factorisation, which rounds differently.  Loop
bounds are the larger env's, the extra iterations masked no-ops.

(a) physics_kernel, every ordered (subject, partner, half) combination of the state catalogue
    (tests/wave_partner_states.py; its CPU test shows that only the legleg / disjoint states can
    have a leg-leg contact) as one wave each, 1 and 5 substeps, contact caps 8 and 16.
    Beside a partner without leg-leg contact: qpos, qvel, qacc_warmstart and the pipeline record
    bit-identical over all such partners and both halves.  Beside a leg-leg partner: inside the
    oracle tolerance of test_gpu_edge._physics_compare (spread 10 beside `disjoint`, as there), the
    oracle's contact set after one substep, and the same bits in both halves.
(b) the same with two Newton iterations (envs of one wave needing different trip counts).
(c) the odd batch's last env, whose half-wave partner is the kernel's clamped clone of it.
(d) env level, a model without leg-leg candidate pairs (the switch cannot happen: bit-identity is
    unconditional): resampling, kicks, terminations and auto-reset at different steps, domain
    randomisation and per-env terrain, 6 steps fused and single-step, under three arrangements of
    the same envs (identity; swapped inside every pair; rotated by one).
(e) the 16-env policy tile: rows moved inside and across tiles, n = 40.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import common
import gpu_harness as G
import wave_partner_states as W
from oracle import oracle as O
from pupperv3_mjx import _abi, _lib, domain_randomization, export, rng, wrappers
from pupperv3_mjx.environment import PupperV3Env, make_keys
from test_gpu_edge import _contact_set

pytestmark = pytest.mark.gpu


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def world(require_gpu, tmp_path_factory):
    path = common.write_model(tmp_path_factory.mktemp("wp"), 10)
    m, _, host = common.env_model_and_config(path)
    jr = host.sys_model.jnt_range
    return SimpleNamespace(path=path, m=m, jr=jr, cat=W.catalogue(m, jr), envs={}, runs={}, oracle={})


@pytest.fixture(scope="module", autouse=True)
def _close_envs(world):
    yield
    for e in world.envs.values():
        e.close()


# ------------------------------------------------------------------------------ the pair layout
def _layout(cat):
    """Every ordered (subject s, partner p, half h) as one wave: (batch states, env[s, p, h] = the
    subject's env index; its partner is env ^ 1)."""
    S = len(cat)
    rows, env = [], np.zeros((S, S, 2), dtype=int)
    for s in range(S):
        for p in range(S):
            for h in (0, 1):
                w = len(rows) // 2
                pair = [cat[s][2], cat[p][2]]
                rows += pair if h == 0 else pair[::-1]
                env[s, p, h] = 2 * w + h
    return W.stack(rows), env


def _physics_bits(e, states, nsteps):
    """(u32 [n, 55 + 304] of qpos | qvel | qacc_warmstart | pipeline record, the f64 arrays)."""
    e._put(_abi.F_PIPELINE, np.zeros((e.num_envs, _abi.PIPE_STRIDE), np.float32))  # this run's record only
    out = G.gpu_physics(e, *states, nsteps)
    assert all(np.all(np.isfinite(x)) for x in out)
    return _u32(np.concatenate(out, axis=1)), out


FIELDS = (("qpos", 0, 19), ("qvel", 19, 37), ("qws", 37, 55), ("pipe", 55, 55 + _abi.PIPE_STRIDE))


def _diff(a, b):
    """Which fields of two bit rows differ, and in how many words."""
    return {k: int((a[lo:hi] != b[lo:hi]).sum()) for k, lo, hi in FIELDS if np.any(a[lo:hi] != b[lo:hi])}


def _pair_run(world, cap, nsteps, iterations=1, categories=W.CATEGORIES):
    """The pair layout of `categories` through physics_kernel (cached): bits, arrays, env index."""
    key = (cap, nsteps, iterations)
    if key not in world.runs:
        cat = [c for c in world.cat if c[1] in categories]
        states, env = _layout(cat)
        n = states[0].shape[0]
        if (cap, iterations) not in world.envs:
            if iterations == 1:
                world.envs[cap, iterations] = PupperV3Env(**common.fixture_kwargs(world.path), num_envs=n,
                                                          max_contacts=cap)
            else:
                m2 = type(world.m).from_buffer_copy(world.m)
                m2.iterations = iterations
                world.envs[cap, iterations] = G.env_with_model(world.path, m2, n)
        e = world.envs[cap, iterations]
        assert e.num_envs == n and n <= 400
        bits, arrays = _physics_bits(e, states, nsteps)
        world.runs[key] = SimpleNamespace(cat=cat, env=env, bits=bits, arrays=arrays)
    return world.runs[key]


def _assert_partner_blind(run):
    """Every subject: the same bits beside every partner without leg-leg contact, in both halves.
    Returns {subject name: its bits}."""
    plain = [p for p, c in enumerate(run.cat) if c[1] not in W.LEGLEG]
    ref, bad = {}, []
    for s, (name, _, _) in enumerate(run.cat):
        r = run.bits[run.env[s, plain[0], 0]]
        ref[name] = r
        for p in plain:
            for h in (0, 1):
                d = _diff(run.bits[run.env[s, p, h]], r)
                if d:
                    bad.append((name, run.cat[p][0], h, d))
    assert not bad, f"{len(bad)} (subject, partner, half) differ from (subject, {run.cat[plain[0]][0]}, 0): {bad[:12]}"
    return ref


def _oracle(world, cap, nsteps, precision):
    key = (cap, nsteps, precision)
    if key not in world.oracle:
        states = W.stack([c[2] for c in world.cat])
        world.oracle[key] = [np.array([O.mj_step(world.m, *(x[i] for x in states), nsteps=nsteps, ncon_max=cap,
                                                 precision=precision)[k] for i in range(len(world.cat))])
                             for k in (0, 1, 3)]
    return world.oracle[key]


# ------------------------------------------------------------------------------ (a) physics level
@pytest.mark.parametrize("cap", [0, 16])
@pytest.mark.parametrize("nsteps", [1, 5])
def test_physics_bits_do_not_depend_on_the_partner(world, nsteps, cap):
    """200 waves, 400 envs.  On an MI355X every one of the 16 (plain subject, leg-leg partner)
    combinations differs bitwise from the subject's result beside a plain partner, as the contract
    allows; the largest difference relative to the field's largest entry (qpos, qvel) is 3.7e-5
    after one substep and 4.3e-5 after five, at both contact caps (the report line)."""
    run = _pair_run(world, cap, nsteps)
    S = len(run.cat)
    assert S == len(world.cat) and run.bits.shape[0] == 4 * S * S
    ref = _assert_partner_blind(run)
    # the catalogue's categories are the kernel's too (contact counts of the first substep)
    if nsteps == 1:
        for s, (name, c, _) in enumerate(run.cat):
            ncon = int(run.arrays[3][run.env[s, 0, 0], _abi.P_NCON])
            assert (ncon == 0) == (c in ("air", "limit")) and (c != "knees" or ncon >= 6), (name, ncon)

    # beside a leg-leg partner: the documented contract
    oq, ov, op = _oracle(world, cap, nsteps, "f64")
    fq, fv, _ = _oracle(world, cap, nsteps, "f32")
    gq, gv, _, gp = run.arrays
    plain = [s for s, c in enumerate(run.cat) if c[1] not in W.LEGLEG]
    differ, rel = 0, 0.0
    for p, (pname, pc, _) in enumerate(run.cat):
        if pc not in W.LEGLEG:
            continue
        spread = 10 if pc == "disjoint" else 5
        for h in (0, 1):
            idx = [run.env[s, p, h] for s in plain]
            # test_gpu_edge._physics_compare's rule on the batch of plain subjects beside this partner
            eq, ev = np.abs(gq[idx] - oq[plain]).max(), np.abs(gv[idx] - ov[plain]).max()
            assert eq <= max(2e-5 * nsteps, spread * np.abs(fq[plain] - oq[plain]).max()), (pname, h, eq)
            assert ev <= max(3e-3, spread * np.abs(fv[plain] - ov[plain]).max()), (pname, h, ev)
            if nsteps == 1:
                for s in plain:
                    assert _contact_set(gp[run.env[s, p, h]]) == _contact_set(op[s]), (run.cat[s][0], pname, h)
        for s, (name, _, _) in enumerate(run.cat):  # (every subject, the leg-leg ones too)
            a, b = run.bits[run.env[s, p, 0]], run.bits[run.env[s, p, 1]]
            assert not _diff(a, b), (name, pname, _diff(a, b))
        for s in plain:
            a, b = run.bits[run.env[s, p, 0]][:55], ref[run.cat[s][0]][:55]
            if np.any(a != b):
                differ += 1
                x, y = a.view(np.float32).astype(np.float64), b.view(np.float32).astype(np.float64)
                rel = max(rel, max(np.abs(x[lo:hi] - y[lo:hi]).max() / np.abs(y[lo:hi]).max() for lo, hi in ((0, 19), (19, 37))))
    G.report("wave_partners_physics", {"nsteps": nsteps, "cap": cap or 8, "waves": 2 * S * S,
                                       "plain_subjects_beside_legleg": 2 * len(plain),
                                       "differ_bitwise_from_plain_result": differ, "max_rel_diff": rel})


# ------------------------------------------------------------------------------ (b) two iterations
ITER2 = ("air", "stand", "knees", "boxes")


def test_two_newton_iterations_bits_do_not_depend_on_the_partner(world):
    """The second iteration is skipped per env once its gradient is small: the two envs of a wave
    then need different trip counts.  Bit-identity only (no claim about convergence)."""
    run = _pair_run(world, 0, 1, iterations=2, categories=ITER2)
    assert {c[1] for c in run.cat} == set(ITER2)
    ref = _assert_partner_blind(run)
    one = _assert_partner_blind(_pair_run(world, 0, 1))
    # the second iteration ran (the 12 frictionloss rows keep even the airborne state from
    # converging in one)
    moved = [name for name in ref if np.any(ref[name][:55] != one[name][:55])]
    assert moved, "two iterations gave every subject the bits of one"
    G.report("wave_partners_iter2", {"waves": 2 * len(run.cat) ** 2, "subjects_changed_by_iteration_2": moved})


# ------------------------------------------------------------------------------ (c) the odd last wave
@pytest.mark.parametrize("nsteps", [1, 5])
def test_last_env_of_an_odd_batch_beside_its_clone(world, nsteps):
    want = _assert_partner_blind(_pair_run(world, 0, nsteps))
    by_name = {c[0]: c for c in world.cat}
    e = PupperV3Env(**common.fixture_kwargs(world.path), num_envs=3)
    try:
        for name in ("air", "knees6", "knees10", "boxes"):
            states = W.stack([by_name["stand"][2], by_name["low"][2], by_name[name][2]])
            bits, _ = _physics_bits(e, states, nsteps)
            assert not _diff(bits[2], want[name]), (name, _diff(bits[2], want[name]))
    finally:
        e.close()


# ------------------------------------------------------------------------------ (d) env level
D_KW = dict(resample_velocity_step=2, kick_probability=0.5, terminal_body_z=0.21)
K_STEPS, EPISODE = 6, 3


def _arrangements(n, tile=None):
    """name -> perm: the arranged batch's row j is env perm[j] of the identity batch."""
    ident = np.arange(n)
    out = {"identity": ident, "rotated": np.roll(ident, -1)}
    if tile is None:
        swap = ident.copy()
        swap[:n // 2 * 2] = ident[:n // 2 * 2].reshape(-1, 2)[:, ::-1].reshape(-1)
        out["swapped"] = swap
    else:
        out["reversed_in_tile"] = np.concatenate([ident[t:t + tile][::-1] for t in range(0, n, tile)])
    for p in out.values():
        assert sorted(p) == list(ident)
    return out


def _unpermute(a, perm, axis=0):
    out = np.empty_like(a)
    idx = [slice(None)] * a.ndim
    idx[axis] = perm
    out[tuple(idx)] = a
    return out


def _flat_model(world, **kw):
    """The 10-box model without leg-leg candidate pairs, with the env constructor's overrides."""
    m, _, _ = common.env_model_and_config(world.path, **kw)
    m2 = W.without_legleg_pairs(m)
    assert m2.npair == m.npair - 24 and not W.legleg_pairs(m2)
    return m2


SLAB_DROP = 0.155  # base height at which the default pose stands on its four feet (common.random_physics_states)


def _terrain(world, m2, keys, seed, **kw):
    """Per-env terrain under where reset puts the envs (a function of their keys):
    common.terrain_under's rails and random boxes, and in slot 2 of two envs out of three a slab
    whose top lies SLAB_DROP below the env's own start height, so those envs stand on a box of
    their own terrain row from the first step on (reset drops the others from 0.18 .. 0.24 m: they
    touch nothing within the few steps run here)."""
    e = G.env_with_model(world.path, m2, len(keys), **kw)
    try:
        pos = e.reset(keys)._record[:, _abi.S_QPOS:_abi.S_QPOS + 3].astype(np.float64)
    finally:
        e.close()
    t = common.terrain_under(pos[:, 0:2], 10, seed=seed)
    for i, (x, y, z) in enumerate(pos):
        if i % 3:
            t[i, 2] = (x, y, z - SLAB_DROP - 0.02, 1, 0, 0, 0, 0.5, 0.5, 0.02)
        else:
            t[i, 2, 7:10] = 0.0
    return t


def _box_contacts(m, pipe):
    """Contacts with a box geom in each pipeline record of pipe[..., 304]."""
    boxes = [int(m.cgeom_id[g]) for g in O.terrain_slots(m)]
    g2 = pipe[..., _abi.P_CON_GEOM + 1:_abi.P_CON_GEOM + 32:2]
    live = np.arange(16) < pipe[..., _abi.P_NCON, None]
    return (np.isin(g2, boxes) & live).sum(axis=-1)


def _device_rows(e):
    return {"record": e._get(_abi.F_STATE), "metrics": e._get(_abi.F_METRICS), "pipeline": e._get(_abi.F_PIPELINE),
            "episode": e._get(_abi.F_EPISODE)}


def _env_run(world, m2, perm, keys, acts, dr, terrain, fused, **kw):
    """K_STEPS wrapper steps of the arranged batch, every output back in identity order:
    (rows, traj).  rows [n, ...]: the reset's obs and record and the device rows after the last
    step; traj [K, n, ...]: obs / reward / done / truncation of each step and, single-step, the
    device rows after each step."""
    e = G.env_with_model(world.path, m2, len(perm), **kw)
    try:
        w = wrappers.wrap(e, episode_length=EPISODE)
        e._put(_abi.F_DR, dr[perm])
        e.set_terrain(terrain[perm])
        st = w.reset(keys[perm])
        rows = {"reset_obs": np.array(st.obs), "reset_record": np.array(st._record)}
        if fused:
            st, t = w.rollout(st, acts[:, perm], truncation=True)
            traj = {k: np.array(t[k]) for k in TRAJ}
        else:
            steps = {k: [] for k in TRAJ + STEP_ROWS}
            for a in acts[:, perm]:
                st = w.step(st, a)
                steps["obs"].append(np.array(st.obs))  # (reading the state issues its launch: one step each)
                steps["reward"].append(np.array(st.reward))
                steps["done"].append(np.array(st.done))
                dev = _device_rows(e)
                steps["truncation"].append(dev["episode"][:, _abi.EP_TRUNCATION].copy())
                for k in STEP_ROWS:
                    steps[k].append(dev[k[len("step_"):]])
            traj = {k: np.stack(v) for k, v in steps.items()}
        rows.update(_device_rows(e))
        np.testing.assert_array_equal(_u32(rows["record"]), _u32(st._record))
        return ({k: _unpermute(v, perm, 0) for k, v in rows.items()}, {k: _unpermute(v, perm, 1) for k, v in traj.items()})
    finally:
        e.close()


TRAJ = ("obs", "reward", "done", "truncation")
STEP_ROWS = ("step_record", "step_metrics", "step_pipeline", "step_episode")


def _assert_same(a, b, what, keys=None):
    for k in keys or a:
        assert a[k].shape == b[k].shape, (what, k)
        bad = np.argwhere(_u32(a[k]) != _u32(b[k]))
        assert bad.size == 0, f"{what}: {k} differs in {len(bad)} words, first at {bad[0].tolist()}"


@pytest.mark.parametrize("n,history", [(12, 2), (11, 2), (12, 3)], ids=["n12", "n11", "n12_h3"])
def test_env_steps_do_not_depend_on_arrangement(world, n, history):
    kw = dict(D_KW, observation_history=history)
    m2 = _flat_model(world, **kw)
    keys = make_keys(21, n)
    acts = np.random.RandomState(5).uniform(-1, 1, size=(K_STEPS, n, 12)).astype(np.float32)
    _, _, host = common.env_model_and_config(world.path, **kw)
    dr = np.ascontiguousarray(domain_randomization.domain_randomize(host.sys, rng.split(rng.PRNGKey(3), n))[0].dr_table(),
                              dtype=np.float32)
    terrain = _terrain(world, m2, keys, 7, **kw)
    runs = {(name, fused): _env_run(world, m2, perm, keys, acts, dr, terrain, fused, **kw)
            for name, perm in _arrangements(n).items() for fused in (True, False)}
    base_rows, base = runs["identity", False]
    for (name, fused), (rows, traj) in runs.items():
        what = f"{name}, {'fused' if fused else 'single-step'} against identity, single-step"
        _assert_same(rows, base_rows, what)
        _assert_same(traj, base, what, TRAJ if fused else None)

    # the run was not vacuous
    done, rec, pipe = base["done"], base["step_record"], base["step_pipeline"]
    first_reset = np.where(done.any(axis=0), done.argmax(axis=0), -1)
    resets = sorted({int(t) for t in first_reset if t >= 0})
    pairs = done[:, :n // 2 * 2].reshape(K_STEPS, -1, 2)
    lone = int((pairs[:, :, 0] != pairs[:, :, 1]).sum())
    kicks = int(np.any(rec[:, :, _abi.S_KICK:_abi.S_KICK + 2] != 0, axis=2).sum())
    cmd = np.concatenate([base_rows["reset_record"][None], rec])[:, :, _abi.S_COMMAND:_abi.S_COMMAND + 3]
    resamples = int(np.any(cmd[1:] != cmd[:-1], axis=2).sum())
    nbox = _box_contacts(m2, pipe)
    G.report("wave_partners_env", {"n": n, "history": history, "first_reset_steps": resets,
                                   "steps_with_one_env_of_a_wave_reset": lone, "kicks": kicks, "resamples": resamples,
                                   "truncations": int(base["truncation"].sum()), "terminations": int((done - base["truncation"]).sum()),
                                   "env_steps_with_contacts": int((pipe[:, :, _abi.P_NCON] > 0).sum()),
                                   "env_steps_on_a_terrain_box": int((nbox > 0).sum()), "env_steps": K_STEPS * n})
    assert len(resets) >= 2, first_reset  # envs auto-reset at different steps
    assert lone >= 1  # a wave with exactly one of its two envs reset
    assert kicks >= 1 and resamples >= 1
    # the DR and terrain rows matter: envs differ in them, and a third of the env steps or more
    # rest on a box of the env's own terrain row while others touch nothing
    assert np.any(dr[0] != dr[1]) and np.any(terrain[0] != terrain[1])
    assert (nbox > 0).sum() >= K_STEPS * n // 3 and (pipe[:, :, _abi.P_NCON] == 0).sum() >= 1


# ------------------------------------------------------------------------------ (e) policy tile
def _sizes(history):
    return [36 * history, 64, 24]


def _policy_setup(world, n):
    m2 = _flat_model(world)
    keys = make_keys(22, n)
    return m2, keys, _terrain(world, m2, keys, 8)


def test_policy_rollout_does_not_depend_on_the_row_in_the_tile(world):
    """pp3_rollout_policy, n = 40 (two whole tiles and a ragged third), K = 3: the deterministic
    policy rollout bit for bit under rotation by one (rows cross tile boundaries and change
    partners) and reversal inside each tile."""
    from test_gpu_policy import _policy
    n, K = 40, 3
    m2, keys, terrain = _policy_setup(world, n)
    dp = export.DevicePolicy(_policy([72, 256, 128, 128, 24], "elu"))
    got = {}
    try:
        for name, perm in _arrangements(n, tile=16).items():
            e = G.env_with_model(world.path, m2, n)
            try:
                assert e._L.pp3_rollout_policy_fused(e._h) == 1
                e.set_terrain(terrain[perm])
                st = e.reset(keys[perm])
                st, traj = e.rollout_policy(st, dp, K)
                out = {k: np.array(traj[k]) for k in ("obs", "action", "reward", "done")}
                out.update(record=e._get(_abi.F_STATE), metrics=e._get(_abi.F_METRICS), pipeline=e._get(_abi.F_PIPELINE))
                got[name] = {k: _unpermute(v, perm, axis=0 if k in ("record", "metrics", "pipeline") else 1)
                             for k, v in out.items()}
            finally:
                e.close()
    finally:
        dp.close()
    for name in got:
        _assert_same(got[name], got["identity"], f"policy rollout, {name} against identity")
    nbox = _box_contacts(m2, got["identity"]["pipeline"])
    G.report("wave_partners_policy", {"n": n, "K": K, "envs_on_a_terrain_box_at_the_end": int((nbox > 0).sum())})
    assert (nbox > 0).sum() >= n // 3 and (nbox == 0).sum() >= 1
    assert np.any(got["identity"]["action"][0, 0] != got["identity"]["action"][0, 1])


def test_sampled_policy_rollout_does_not_depend_on_the_row_in_the_tile(world):
    """pp3_rollout_policy_sample, n = 40, K = 3.  An env's noise word depends on its row, so its
    sampled actions differ between arrangements by design.  What must not: the logits of the first
    step's observations (pp3_policy_sample on the reset observations, rows permuted), and the env
    outputs given the actions -- every arrangement's trajectory, un-permuted, equals a plain
    pp3_rollout of the identity batch on that arrangement's own un-permuted actions."""
    from test_gpu_ppo_targets import _training
    n, K = 40, 3
    m2, keys, terrain = _policy_setup(world, n)
    dp = export.DevicePolicy(_training([72, 64, 24]))
    lb, ab = _lib.DeviceBuffer(4 * n * 24), _lib.DeviceBuffer(4 * n * 12)
    got, replay, actions = {}, {}, []
    try:
        for name, perm in _arrangements(n, tile=16).items():
            e, e2 = G.env_with_model(world.path, m2, n), G.env_with_model(world.path, m2, n)
            try:
                assert e._L.pp3_rollout_policy_fused(e._h) == 1
                e.set_terrain(terrain[perm])
                st = e.reset(keys[perm])
                dp.sample_env(e, rng.PRNGKey(9), ab.ptr.value, logits_dev=lb.ptr.value)
                e.synchronize()
                logits = np.zeros((n, 24), np.float32)
                lb.download(logits)
                st, traj, _ = e.rollout_policy_sample(st, dp, K, rng.PRNGKey(9))
                out = {k: np.array(traj[k]) for k in ("obs", "action", "reward", "done")}
                out.update(record=e._get(_abi.F_STATE), logits=logits)
                got[name] = {k: _unpermute(v, perm, axis=0 if k in ("record", "logits") else 1) for k, v in out.items()}
                actions.append(got[name]["action"])
                # the identity batch stepped on these actions
                e2.set_terrain(terrain)
                s2, t2 = e2.rollout(e2.reset(keys), got[name]["action"])
                replay[name] = {k: np.array(t2[k]) for k in ("obs", "reward", "done")}
                replay[name]["record"] = e2._get(_abi.F_STATE)
            finally:
                e.close()
                e2.close()
    finally:
        dp.close()
        lb.free()
        ab.free()
    for name in got:
        _assert_same(got[name], got["identity"], f"sampled rollout logits, {name} against identity", ("logits",))
        _assert_same(got[name], replay[name], f"sampled rollout, {name}, against pp3_rollout on its actions",
                     ("obs", "reward", "done", "record"))
    assert np.any(actions[0] != actions[1])  # (the noise does follow the row)
