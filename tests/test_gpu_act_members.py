"""The member acting kernel and the batched greedy evaluation of the 2-D environments (csrc/act_members.hip:
pdec_policy_act_members; csrc/rollout.hip: pdec_rollout_members, served = 2; population.py: evaluate_actors).  Served means bit
for bit: a member's actions are its solo pdec_policy_act_rng call's, a trajectory's env step does not depend on the batch it
sits in, and so a member's rollout rows are those of its solo rollout on a B = K environment."""
import ctypes as C
import importlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"f32": torch.float32, "f64": torch.float64}


def _mod(pkg, name):
    return importlib.import_module(pkg.__name__ + "." + name)


def _bits(t):
    t = t.contiguous()
    return t.view({8: torch.int64, 4: torch.int32}[t.element_size()])


def _same(a, b):
    """torch.equal on the bit patterns (NaN-safe, and -0.0 != 0.0)"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _setup(pkg, which):
    if which == "fluid2":
        return pkg.FluidSetup(nx=64, oversampling=3)
    if which == "fluid3":
        return pkg.FluidSetup(nx=64, oversampling=3, drop_middle_layer=False)
    assert which == "kseg2d"
    return pkg.KellerSegel2DSetup(nx=64, ny=64, substeps=4)


def _actors(pkg, setup, n, dtype=torch.float32, acts=None):
    """n distinct actors of the setup's shape (create_agent's layer table and initialiser) with non-zero biases"""
    nna = _mod(pkg, "nna")
    out = []
    for m in range(n):
        rng = np.random.default_rng(500 + m)
        a = nna.create_chain(na=1, ns=setup.state_shape[0], is_actor=True, init_rng=rng, nna_scale=setup.nna_scale,
                             drop_middle_layer=setup.drop_middle_layer)
        if acts is not None:
            a = nna.HipMLP(a.dims, acts, a.params())
        P = a.params()
        a.set_params([p if p.ndim == 2 else rng.uniform(-0.3, 0.3, p.shape).astype(p.dtype) for p in P])
        out.append(a if dtype == torch.float32 else a.clone(dtype=dtype))
    return out


def _handles(pkg, models):
    return (pkg._lib.Handle * len(models))(*[int(getattr(m.handle, "value", m.handle)) for m in models])


def _route(pkg, model, cols):
    name, lds = C.create_string_buffer(128), C.c_int64(0)
    pkg._lib.check(model.lib.pdec_debug_batched_update_route(model.handle, 0, 0, 0, int(cols), 4, name, 128, C.byref(lds)))
    return name.value.decode()


def _plan(pkg, model, state_dtype, cols):
    tc, nt, lds = C.c_int(-1), C.c_int(-1), C.c_int64(-1)
    pkg._lib.check(model.lib.pdec_debug_act_members_plan(model.handle, pkg._lib.dtype_code(state_dtype), int(cols), C.byref(tc),
                                                         C.byref(nt), C.byref(lds)))
    return tc.value, nt.value, lds.value


CANARY, SLACK = 12345.678, 512


def _act_members(pkg, env, models, state, cols, lim):
    """the member call on a canary-filled buffer with slack on both sides -> (served, actions [M cols, no], buffer intact outside)"""
    no = models[0].dims[-1]
    n = len(models) * cols * no
    buf = torch.full((n + 2 * SLACK,), CANARY, dtype=state.dtype, device=DEV)
    served = C.c_int(-1)
    rc = env.lib.pdec_policy_act_members(env.handle, _handles(pkg, models), len(models), pkg._lib.ptr(state), int(cols), float(lim),
                                         pkg._lib.ptr(buf[SLACK:]), C.byref(served))
    torch.cuda.synchronize()
    assert rc == 0, env.lib.pdec_last_error()
    fill = torch.full((SLACK,), CANARY, dtype=state.dtype, device=DEV)
    intact = _same(buf[:SLACK], fill) and _same(buf[SLACK + n:], fill)
    return served.value, buf[SLACK:SLACK + n].view(len(models) * cols, no), intact


def _solo_act(pkg, clone, state, cols, lim):
    out = torch.empty((cols, clone.dims[-1]), dtype=state.dtype, device=DEV)
    pkg._lib.check(clone.lib.pdec_policy_act_rng(clone.handle, pkg._lib.ptr(state), int(cols), 0.0, float(lim), 0, 0, 0,
                                                 pkg._lib.ptr(out)))
    return out


# ---------------------------------------------------------------------------------------------- 1. the acting entry

@pytest.mark.parametrize("pair", ["f64_f32", "f64_f64", "f32_f32"])
@pytest.mark.parametrize("which", ["fluid2", "fluid3", "kseg2d"])
def test_member_actions_equal_solo_calls(pkg, which, pair):
    """pdec_policy_act_members against M greedy pdec_policy_act_rng calls on clones of the states' dtype, bit for bit: M in
    {1, 3, 5}, C around 64 and around the tile width TC of the library's own plan (which must be population.act_members_tiles'),
    act_limit 1.0 and 0.05 (the clamp binds), nothing written outside [0, M C no).  fp32 states: where the solo call takes a
    fused MFMA kernel (another summation order) the entry must answer served = 0 instead."""
    sd, pd = (DT[x] for x in pair.split("_"))
    setup = _setup(pkg, which)
    ns = setup.state_shape[0]
    env = pkg.PDEenv(setup, B=1, dtype=sd, autoreset=False)
    members = _actors(pkg, setup, 5, dtype=pd)
    maxw, isz = max(members[0].dims), torch.empty((), dtype=sd).element_size()
    tiles_of = _mod(pkg, "population").act_members_tiles
    TC = tiles_of(10 ** 6, maxw, isz)[0]
    assert TC >= 64 and 2 * maxw * TC * isz <= 48 * 1024 < 2 * maxw * (TC + 64) * isz
    Cs = sorted({1, 63, 64, 65, TC - 1, TC, TC + 1, 2 * TC + 3})
    clones = [m.clone(dtype=sd, max_cols=max(Cs)) for m in members]
    g = torch.Generator(device="cpu").manual_seed(7)
    states = [torch.randn((max(Cs), ns), generator=g, dtype=torch.float64).to(device=DEV, dtype=sd) for _ in members]
    n_served = n_clamped = 0
    for cols in Cs:
        tc, nt, lds = _plan(pkg, members[0], sd, cols)
        assert (tc, nt) == tiles_of(cols, maxw, isz) and lds == 2 * maxw * tc * isz, (cols, tc, nt, lds)
        fused = sd == torch.float32 and _route(pkg, clones[0], cols).startswith("policy_act")
        for lim in (1.0, 0.05):
            solo = [_solo_act(pkg, c, s[:cols].contiguous(), cols, lim) for c, s in zip(clones, states)]
            for M in (1, 3, 5):
                state = torch.cat([s[:cols] for s in states[:M]]).contiguous()
                served, act, intact = _act_members(pkg, env, members[:M], state, cols, lim)
                assert intact, (cols, lim, M)
                if fused:
                    assert served == 0 and bool((act == CANARY).all()), (cols, lim, M)
                    continue
                assert served == 1, (cols, lim, M)
                n_served += 1
                for m in range(M):
                    assert _same(act[m * cols:(m + 1) * cols], solo[m]), (cols, lim, M, m)
                if lim == 0.05:
                    assert bool((act.abs() <= 0.05).all())
                    n_clamped += int((act.abs() == 0.05).sum())
                if M >= 2 and cols >= 63:      # the members differ: a table that served member 0's actor to all would show
                    assert not _same(act[:cols], act[cols:2 * cols])
    assert n_clamped > 0 or n_served == 0, "the clamp never bound"
    if sd == torch.float64:
        assert n_served == len(Cs) * 2 * 3          # fp64 states are always served
    elif which != "fluid3":                         # (the 3-layer fp32 actor acts through the fused 3-layer kernel at any width)
        assert n_served >= 4 * 2 * 3, n_served      # 2-layer fp32: fused from 256 columns on only


@pytest.mark.parametrize("first_act", ["relu", "tanh"])
def test_nan_in_one_column_stays_in_that_column(pkg, first_act):
    """a NaN in one state column of the middle member (fp64 states, Float32 actors, M = 3, C = 65): every other column keeps its
    bits, and the column itself gets what the solo call gives it.  With the shipped relu hidden layer that is a NUMBER -- relu is
    z > 0 ? z : 0, which maps NaN to 0 in every forward pass of the library --; with a tanh hidden layer the action is NaN."""
    setup = _setup(pkg, "fluid2")
    ns, cols, M = setup.state_shape[0], 65, 3
    env = pkg.PDEenv(setup, B=1, dtype=torch.float64, autoreset=False)
    members = _actors(pkg, setup, M, acts=[first_act, "tanh"])
    g = torch.Generator(device="cpu").manual_seed(11)
    state = torch.randn((M * cols, ns), generator=g, dtype=torch.float64).to(DEV)
    served, clean, intact = _act_members(pkg, env, members, state, cols, 1.0)
    assert served == 1 and intact and bool(torch.isfinite(clean).all())
    hot = cols + 64                                  # the middle member's last column: the partial second tile
    bad = state.clone()
    bad[hot, 4] = float("nan")
    served, act, intact = _act_members(pkg, env, members, bad, cols, 1.0)
    assert served == 1 and intact
    keep = torch.ones(M * cols, dtype=torch.bool, device=DEV)
    keep[hot] = False
    assert _same(act[keep], clean[keep])
    solo = _solo_act(pkg, members[1].clone(dtype=torch.float64, max_cols=cols), bad[cols:2 * cols].contiguous(), cols, 1.0)
    assert _same(act[cols:2 * cols], solo)
    assert bool(torch.isnan(act[hot]).all()) == (first_act == "tanh")


# ---------------------------------------------------------------------------------------------- 2. refusals

def test_refusals_enqueue_nothing(pkg):
    setup2, setup3 = _setup(pkg, "fluid2"), _setup(pkg, "fluid3")
    ns = setup2.state_shape[0]
    env64 = pkg.PDEenv(setup2, B=1, dtype=torch.float64, autoreset=False)
    env32 = pkg.PDEenv(setup2, B=1, dtype=torch.float32, autoreset=False)
    a2, a3 = _actors(pkg, setup2, 2), _actors(pkg, setup3, 1)
    s64 = torch.randn((2 * 256, ns), dtype=torch.float64, device=DEV)
    s32 = s64.float()
    # differing shapes
    served, act, intact = _act_members(pkg, env64, [a2[0], a3[0]], s64, 64, 1.0)
    assert served == 0 and intact and bool((act == CANARY).all())
    # differing dtypes of the members
    served, act, intact = _act_members(pkg, env64, [a2[0], a2[1].clone(dtype=torch.float64)], s64, 64, 1.0)
    assert served == 0 and intact and bool((act == CANARY).all())
    # an fp64 actor under fp32 states
    served, act, intact = _act_members(pkg, env32, [a.clone(dtype=torch.float64) for a in a2], s32, 64, 1.0)
    assert served == 0 and intact and bool((act == CANARY).all())
    # fp32 states where the solo call is a fused MFMA kernel: 2-layer from 256 columns on, 3-layer at any width
    assert _route(pkg, a2[0], 256).startswith("policy_act2_kernel") and _route(pkg, a3[0], 64).startswith("policy_act_fused_kernel")
    served, act, intact = _act_members(pkg, env32, a2, s32, 256, 1.0)
    assert served == 0 and intact and bool((act == CANARY).all())
    served, act, intact = _act_members(pkg, env32, a3, s32, 64, 1.0)
    assert served == 0 and intact and bool((act == CANARY).all())
    # ... while 255 columns are served (small_act_kernel or the generic launches: the member kernel's arithmetic)
    assert _route(pkg, a2[0], 255) in ("small_act_kernel", "generic")
    served, act, intact = _act_members(pkg, env32, a2, s32, 255, 1.0)
    assert served == 1 and intact
    # a layer too wide for one tile of 64 columns (fp64: 2 * 49 * 64 * 8 B > 48 KiB)
    nna = _mod(pkg, "nna")
    wide = [nna.HipMLP([ns, 49, 1], ["relu", "tanh"], nna.glorot_uniform(np.random.default_rng(m), [ns, 49, 1])) for m in range(2)]
    assert _plan(pkg, wide[0], torch.float64, 64)[0] == 0
    served, act, intact = _act_members(pkg, env64, wide, s64, 64, 1.0)
    assert served == 0 and intact and bool((act == CANARY).all())


# ---------------------------------------------------------------------------------------------- 3. the env step and B

def _env_layout(setup, y0):
    """setup.generate_random_init's host fields in the environment's memory layout (float64)"""
    y0 = np.asarray(y0)
    if getattr(setup, "is_fluid", False):          # complex [B, ny, nx] -> [B, nx, ny, (re, im)]
        z = np.swapaxes(y0, -1, -2)
        return torch.as_tensor(np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1)))
    return torch.as_tensor(np.ascontiguousarray(np.moveaxis(y0, 1, -1)))      # [B, 2, ny, nx] -> [B, ny, nx, 2]


def _forced_steps(pkg, setup, dtype, y0, acts):
    """pdec_env_step with the given actions [T, B, A, 1] from y0 [B, ...]: per step (y, p, state, reward, done)"""
    B = y0.shape[0]
    env = pkg.PDEenv(setup, B=B, dtype=dtype, y0=y0, autoreset=False)
    P, kw = pkg._lib.ptr, dict(dtype=dtype, device=DEV)
    y, st, ap = env.y.clone(), env.state.clone(), torch.zeros(env._ashape, **kw)
    rows = []
    for t in range(acts.shape[0]):
        a = acts[t].to(dtype).contiguous()
        y2, p, st2 = torch.empty_like(y), torch.empty(env._pshape, **kw), torch.empty_like(st)
        r, d = torch.empty((B, setup.reward_len), **kw), torch.zeros(B, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        pkg._lib.check(env.lib.pdec_env_step(env.handle, P(y), P(a), P(ap), P(st), P(y2), P(p), P(st2), P(r), P(d)))
        torch.cuda.synchronize()
        rows.append(dict(y=y2, p=p, state=st2, reward=r, done=d))
        y, st, ap = y2, st2, a
    print(f"part streams of the step ({type(setup).__name__}, B = {B}, {dtype}): {env.n_part_streams}")
    env.close()
    return rows


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("which,M,K", [("fluid2", 3, 3), ("kseg2d", 3, 2)])
def test_env_step_does_not_depend_on_the_batch(pkg, which, M, K, dtype):
    """three teacher-forced control steps of B = M K trajectories (fluid: 9, an odd batch; 2-D Keller-Segel: 6) against the same
    trajectories stepped as M batches of K: y, p, state, reward and the done flags bit for bit.  This is what lets a member's
    block of the B = M K evaluation environment stand for its solo B = K environment."""
    setup = _setup(pkg, which)
    rng = np.random.default_rng(3)
    y0 = _env_layout(setup, setup.generate_random_init(rng, M * K)).to(DEV)
    A = setup.state_shape[1]
    acts = torch.as_tensor(rng.uniform(-1, 1, (3, M * K, A, 1))).to(DEV)
    big = _forced_steps(pkg, setup, DT[dtype], y0, acts)
    for m in range(M):
        sl = slice(m * K, (m + 1) * K)
        small = _forced_steps(pkg, setup, DT[dtype], y0[sl].contiguous(), acts[:, sl].contiguous())
        for t in range(3):
            for k in ("y", "p", "state", "reward", "done"):
                assert _same(big[t][k][sl], small[t][k]), (m, t, k)
    assert not _same(big[2]["y"][:K], big[2]["y"][K:2 * K])          # (the blocks differ)
    assert bool(torch.isfinite(big[2]["y"]).all()) and not bool(torch.cat([r["done"] for r in big]).any())


def test_batch_independence_holds_with_the_batch_split_into_parts():
    """the same comparison with the step's part-batch children forced on (PDEC_FLUID_SPLIT=2: B = 9 steps as 4 + 5 trajectories
    on two streams, B = 3 as 1 + 2; PDEC_KSEG2D_SPLIT=2 for the fp32 2-D Keller-Segel sub-steps).  By default the fluid step
    splits from the padded 512-point grid and 8 trajectories on, which an evaluation at B = M K reaches where its solo
    rollouts at B = K do not.  The switches are read once per process, hence the fresh one."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, PDEC_FLUID_SPLIT="2", PDEC_KSEG2D_SPLIT="2")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-s", "-p", "no:cacheprovider",
                        "-k", "test_env_step_does_not_depend_on_the_batch"], env=env, capture_output=True, text=True, timeout=300,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "4 passed" in r.stdout, r.stdout[-2000:]
    assert "part streams of the step (FluidSetup, B = 9, torch.float64): 1" in r.stdout, r.stdout[-2000:]
    assert "part streams of the step (FluidSetup, B = 3, torch.float32): 1" in r.stdout, r.stdout[-2000:]


# ---------------------------------------------------------------------------------------------- 4. - 6. rollouts

_cache = {}


def _case(pkg, which, dtype):
    """(setup, actors, y0 in the environment's layout, M, K) of a rollout case, and its evaluation + solo rollouts, made once"""
    key = (which, dtype)
    if key not in _cache:
        setup = _setup(pkg, which)
        M, K = (3, 3) if which.startswith("fluid") else (3, 2)
        y0 = _env_layout(setup, setup.generate_random_init(np.random.default_rng(17), K)).to(DEV)
        actors = _actors(pkg, setup, M)
        res = pkg.evaluate_actors(setup, actors, y0=y0, steps=3, dtype=DT[dtype], log=True)
        solos = [_solo(pkg, setup, a, y0, 3, DT[dtype]) for a in actors]
        _cache[key] = dict(setup=setup, M=M, K=K, y0=y0, actors=actors, res=res, solos=solos)
    return _cache[key]


def _solo(pkg, setup, actor, y0, T, dtype):
    env = pkg.PDEenv(setup, B=y0.shape[0], dtype=dtype, y0=y0, autoreset=False)
    out = env.rollout(actor.clone(dtype=env.dtype, max_cols=y0.shape[0] * setup.state_shape[1]), T, learning=False, log=True)
    torch.cuda.synchronize()
    env.close()
    return out


def _assert_member_equals_solo(res, m, solo, rows=None):
    """_assert_members_equal_solo of tests/test_gpu_population_eval.py for one member (rows: the trajectories compared)"""
    rows = slice(None) if rows is None else rows
    for k in ("y", "p", "action", "reward"):
        assert _same(res[k][:, m][:, rows], solo[k][:, rows]), (m, k)
    assert _same(res["reward_sum"][m][rows], solo["reward_sum"][rows]), m
    assert torch.equal(res["done_step"][m][rows], solo["done_step"][rows]), m
    assert _same(res["episode_reward"][m][rows], solo["reward_sum"].mean(dim=1)[rows]), m


@pytest.mark.parametrize("which,dtype", [("fluid2", "f64"), ("fluid3", "f64"), ("kseg2d", "f64"), ("fluid2", "f32")])
def test_batched_rollouts_equal_solo_rollouts(pkg, which, dtype):
    """evaluate_actors on the 2-D setups: ONE step loop on the B = M K environment (batched), every member's y, p, action, reward,
    reward_sum, done_step and episode_reward bit for bit those of PDEenv(B = K).rollout(actor.clone(dtype = env.dtype))"""
    c = _case(pkg, which, dtype)
    res, M, K = c["res"], c["M"], c["K"]
    if dtype == "f32":      # the solo acting route at these K A columns sums as the member kernel does
        cols = K * c["setup"].state_shape[1]
        assert cols == 192 and _route(pkg, c["actors"][0], cols) in ("small_act_kernel", "generic")
    assert res["batched"] is True and res["one_launch"] is False and res["workgroups"] is None
    assert res["y"].shape[:3] == (3, M, K) and res["action"].shape[:3] == (3, M, K) and res["reward_sum"].shape[:2] == (M, K)
    for m in range(M):
        _assert_member_equals_solo(res, m, c["solos"][m])
    assert not _same(res["action"][:, 0], res["action"][:, 1])
    assert bool((res["done_step"] == -1).all()) and np.isfinite(res["score"]).all()
    assert sorted(res["order"]) == list(range(M))


def _blow_up_scale(setup, y0_row):
    """the factor on one initial field that raises the blow-up flag within three control steps, chosen with the fp64 oracle's
    integrator under zero action, with a margin of 2 on the bound (the actions move the field far less than that)"""
    if getattr(setup, "is_fluid", False):
        from oracle import fluid
        cfg = fluid.FluidConfig(nx=setup.nx, oversampling=setup.oversampling)

        def flagged(y):
            with np.errstate(all="ignore"):
                for _ in range(3):
                    y = fluid.do_step(cfg, y, 0.0)
                    r = fluid.reward_function(cfg, y, np.zeros((1, setup.n_actuators)), np.zeros((1, setup.n_actuators)))
                    if not (np.abs(r) <= 2 * setup.max_value).all():      # check_max_value = "reward"
                        return True
            return False
    else:
        from oracle import keller_segel2d as k2
        cfg = k2.KSeg2DConfig(nx=setup.nx, ny=setup.ny, Lx=setup.Lx, sensor_x=setup.sensor_x, sensor_y=setup.sensor_y,
                              substeps=setup.oversampling)

        def flagged(y):
            with np.errstate(all="ignore"):
                for _ in range(3):
                    y = k2.do_step(cfg, y, np.zeros((setup.ny, setup.nx)))
                    if not (np.abs(y) <= 2 * setup.max_value).all():      # check_max_value = "y"
                        return True
            return False
    for s in (10.0, 100.0, 1e3, 1e4, 1e5):
        if flagged(s * y0_row):
            return s
    raise AssertionError("no scale up to 1e5 leaves the bound within three oracle steps")


@pytest.mark.parametrize("which", ["fluid2", "kseg2d"])
def test_a_blown_up_trajectory_is_its_members_only(pkg, which):
    """initial field 1 scaled (the scale from the oracle's step) so that its blow-up flag rises within the three steps -- the
    environment's ordinary blow-up path.  The members share the fields, so each member's trajectory 1 is flagged, at its solo
    rollout's step; every member scores NaN; all other trajectories keep the bits of the evaluation on the unscaled fields."""
    c = _case(pkg, which, "f64")
    setup, M, K, ok = c["setup"], c["M"], c["K"], c["res"]
    y0_host = setup.generate_random_init(np.random.default_rng(17), K)
    assert _same(_env_layout(setup, y0_host).to(DEV), c["y0"])
    s = _blow_up_scale(setup, y0_host[1])
    y_bad = c["y0"].clone()
    y_bad[1] *= s
    bad = pkg.evaluate_actors(setup, c["actors"], y0=y_bad, steps=3, log=True)
    assert bad["batched"] is True
    assert bool((bad["done_step"][:, 1] >= 0).all()), (s, bad["done_step"])
    others = [k for k in range(K) if k != 1]
    assert bool((bad["done_step"][:, others] == -1).all())
    for m in range(M):
        _assert_member_equals_solo(bad, m, _solo(pkg, setup, c["actors"][m], y_bad, 3, torch.float64))
        _assert_member_equals_solo(bad, m, c["solos"][m], rows=others)
    for k in ("y", "p", "action", "reward"):
        assert _same(bad[k][:, :, others], ok[k][:, :, others]), k
    assert np.isnan(bad["score"]).all() and bad["order"] == list(range(M))


def test_evaluation_leaves_the_actors_alone_and_repeats(pkg):
    c = _case(pkg, "fluid2", "f64")
    before = [[p.copy() for p in a.params()] for a in c["actors"]]
    again = pkg.evaluate_actors(c["setup"], c["actors"], y0=c["y0"], steps=3, log=True)
    assert again["batched"] is True
    for k in ("y", "p", "action", "reward", "reward_sum", "done_step", "episode_reward"):
        assert _same(again[k], c["res"][k]), k
    assert np.array_equal(again["score"], c["res"]["score"]) and again["order"] == c["res"]["order"]
    for a, P in zip(c["actors"], before):
        for x, y in zip(a.params(), P):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    # the default fields (n_inits draws of the environment's own initialiser) take the batched route as well
    k2 = _case(pkg, "kseg2d", "f64")
    r1 = pkg.evaluate_actors(k2["setup"], k2["actors"], n_inits=2, init_seed=5, steps=2)
    r2 = pkg.evaluate_actors(k2["setup"], k2["actors"], n_inits=2, init_seed=5, steps=2)
    assert r1["batched"] is True and _same(r1["reward_sum"], r2["reward_sum"]) and "y" not in r1


# ---------------------------------------------------------------------------------------------- 7. the other routes

@pytest.mark.parametrize("persistent", ["1", "0"])
def test_ks_routes_answer_as_before(pkg, monkeypatch, persistent):
    monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", persistent)
    setup = pkg.KSSetup.KS22()
    agents = [pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(100 + m)) for m in range(2)]
    res = pkg.evaluate_actors(setup, [a.policy.behavior_actor for a in agents], n_inits=2, init_seed=3, steps=4)
    assert res["one_launch"] is (persistent == "1") and res["batched"] is False
    assert res["workgroups"] == (2 if persistent == "1" else None)
