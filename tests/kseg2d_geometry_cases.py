"""The case table of test_gpu_kseg2d_geometry.py: geometries of the 2-D Keller-Segel environment (csrc/kseg2d.hip:
kseg2d_rk4_kernel<T, NSUB, MODE>, kseg2d_actuate_kernel, kseg2d_boxsum_kernel, kseg2d_feat_kernel, kseg2d_terminal_kernel, the
split batch of k2_integrate and the tables pdec_kseg2d_env_create builds) away from the one shipped point (256 x 256 cells, 52 x 52
sensors every 8 cells, border 2, window 3, temporal_steps 2, 32 sub-steps), plus a plain-Python restatement of the host rules
that decide what a geometry reaches (tiles per trajectory, the XCD-aware tile order, the parts of a split batch, the cells of a
clipped box, the launch list of the two-sub-step variant).  Imports numpy only, so test_kseg2d_geometry_table.py holds every claim
of the table against the oracle and the setup's host tables without a GPU.

Every row keeps dx = 0.1 (the shipped cell size) and at least 3 sub-steps of dt = 0.006: with h = dt / substeps the explicit RK4
step on the 5-point Laplacian is stable for about 8 h / dx^2 < 2.78, which 3 sub-steps meet (1.6) and 1 does not (4.8).  nx is a
multiple of 4 (pdec_kseg2d_env_create), actuator boxes are disjoint (it refuses overlap), sensor boxes may overlap."""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "nx ny sensor_x sensor_y border a2s window_size temporal_steps substeps action_punish "
                          "delta_action_punish check_max_value max_value B precs")

HW = 2                           # half window of every box: 5 x 5 cells where the domain does not clip it
TX = 64                          # csrc/kseg2d.hip: K2_TX
BLOWUP_REWARD_MAX = 0.05         # max_value of the "reward" form: tame rewards stay below 2e-3, a patched corner box gives 0.8


def _grid_a2s(Sx, ixs, iys):
    """1-based actuator list of the sensors (iy, ix), 0-based grid indices, row-major over the Sy x Sx sensor grid"""
    return tuple(int(iy) * Sx + int(ix) + 1 for iy in iys for ix in ixs)


def _case(nx, ny, sensor_x=None, sensor_y=None, border=2, a2s=None, window_size=3, temporal_steps=2, substeps=3,
          action_punish=0.0, delta_action_punish=0.0, check_max_value="y", max_value=20.0, B=3, precs=("f64", "f32")):
    sx = range(3, nx + 1, 5) if sensor_x is None else sensor_x
    sy = range(3, ny + 1, 5) if sensor_y is None else sensor_y
    return Case(int(nx), int(ny), tuple(int(s) for s in sx), tuple(int(s) for s in sy), int(border),
                None if a2s is None else tuple(int(a) for a in a2s), window_size, temporal_steps, substeps, action_punish,
                delta_action_punish, check_max_value, max_value, B, tuple(precs))


_CLIP_X = list(range(1, 62, 5)) + [64]                    # 1, 6, ..., 61, 64: boxes 1..3 | 4..8 | ... | 59..63 | 62..64
_CLIP_Y = [1, 6, 11, 16, 20]                              # boxes 1..3 | 4..8 | 9..13 | 14..18 | 18..20
# a non-monotone list on the 20 x 4 sensor grid of 100 x 20 cells (sensor = iy * 20 + ix + 1)
_PERMUTED = [57, 3, 80, 22, 41, 19, 64, 1, 38, 75, 10, 49, 26, 61, 33, 12]

CASES = {
    # ---- the tile kernel: tiles per trajectory, ragged last tiles, the tile order
    "smallest_4x1": _case(4, 1, [2], [1], border=0),      # pdec_kseg2d_env_create's floor; the one box is the whole domain
    "onetile_64x64": _case(64, 64),                       # fp32 exactly one tile; fp64 two tiles with a halo across row 32
    "ragged_68x65": _case(68, 65),                        # last tile column one strip wide, last tile row one row high
    "remap_192x64": _case(192, 64, B=8),                  # 3 / 6 tiles x 8 trajectories: the remap interleaves trajectories
    "noremap_192x64": _case(192, 64),                     # 9 / 18 workgroups: the branch not taken
    # ---- the box sums: a second pass of the column loop, of the sensor loop, clipped boxes
    "wide_260x12": _case(260, 12, border=0),              # nx > 256; the last box ends on cell 260 and is an actuator
    "dense_200x8": _case(200, 8, range(3, 199, 3), [3, 8], border=0, a2s=_grid_a2s(66, range(1, 66, 2), [0, 1])),
    "clipped_64x20": _case(64, 20, _CLIP_X, _CLIP_Y, border=0, a2s=_grid_a2s(14, list(range(12)) + [13], [0, 1, 2, 4])),
    "permuted_100x20": _case(100, 20, a2s=_PERMUTED, action_punish=0.3, delta_action_punish=0.7),
    # ---- ftab: other windows and stacks
    "w1_t3_64x32": _case(64, 32, window_size=1, temporal_steps=3),
    "w5_t1_100x40": _case(100, 40, window_size=5, temporal_steps=1),
    "w3_sy2_64x10": _case(64, 10),                        # Sy = 2 < window: the circular window visits a sensor row twice
    # ---- the other blow-up tests (border 0: the corner box, which the blow-up patch lies under, is an actuator's)
    "rewardcheck_68x65": _case(68, 65, border=0, check_max_value="reward", max_value=BLOWUP_REWARD_MAX),
    "nocheck_68x65": _case(68, 65, check_max_value="off"),
    # ---- the split batch (fp32, one sub-step per launch)
    "split3_68x65": _case(68, 65, B=385, precs=("f32",)),  # 4 tiles x 385 = 1540 >= 1536: parts of 128 / 128 / 129
    "split2_68x65": _case(68, 65, B=256, precs=("f32",)),  # 1024 tiles: two parts of 128
}

NSUB2 = ["ragged_68x65", "onetile_64x64", "remap_192x64"]                 # test c
BLOWUP = ["ragged_68x65", "smallest_4x1", "wide_260x12", "rewardcheck_68x65"]   # test d
SPLIT = {"split3_68x65": 2, "split2_68x65": 1}                            # test e: row -> n_part_streams
GATHER = ["ragged_68x65", "remap_192x64"]                                 # test f
BLOWUP_B = 5


def case_of(case):
    return CASES[case] if isinstance(case, str) else case


# ------------------------------------------------------------------ builders
def build(pkg, k2, case, **override):
    """(pkg.KellerSegel2DSetup, oracle KSeg2DConfig) of a row, both from the same numbers"""
    c = case_of(case)._replace(**override)
    sx, sy = np.array(c.sensor_x, dtype=np.int64), np.array(c.sensor_y, dtype=np.int64)
    a2s = None if c.a2s is None else np.array(c.a2s, dtype=np.int64)
    both = dict(nx=c.nx, ny=c.ny, Lx=0.1 * c.nx, sensor_x=sx, sensor_y=sy, half_window=HW, window_size=c.window_size,
                temporal_steps=c.temporal_steps, substeps=c.substeps, action_punish=c.action_punish,
                delta_action_punish=c.delta_action_punish, max_value=c.max_value)
    setup = pkg.KellerSegel2DSetup(border=c.border, check_max_value=c.check_max_value, actuators_to_sensors=a2s, **both)
    return setup, k2.KSeg2DConfig(border_x=c.border, a2s=a2s, **both)


def n_actuators(case):
    c = case_of(case)
    if c.a2s is not None:
        return len(c.a2s)
    Sx, Sy = len(c.sensor_x), len(c.sensor_y)
    by = min(c.border, (Sy - 1) // 2)
    return (Sx - 2 * c.border) * (Sy - 2 * by)


def inputs(case, B=None, steps=3, seed=0):
    """deterministic inputs of a row: y0 [B, 2, ny, nx] = 1 + 0.05 randn (the oracle's layout), actions [steps, B, 1, A] and the
    previous action [B, 1, A] uniform in [-1, 1]; every trajectory has a field of its own"""
    c = case_of(case)
    B = c.B if B is None else B
    A = n_actuators(c)
    rng = np.random.default_rng([seed, c.nx, c.ny, A])
    y0 = 1.0 + 0.05 * rng.standard_normal((B, 2, c.ny, c.nx))
    return y0, rng.uniform(-1, 1, (steps, B, 1, A)), rng.uniform(-1, 1, (B, 1, A))


PATCH = 40.0


def patch(y, b):
    """u of trajectory b set to 40 on the last two rows and columns (the whole row where the grid is one row high): after one
    control step of 3 or 5 sub-steps the oracle's field is finite with max |y| between 28 and 38 -- the u - u^2 term takes 40
    down to about 37, diffusion out of a 2 x 2 patch further, the more so beside a forced box; a 1 x 1 patch decays to 17 - 22
    and is not usable"""
    if y.shape[2] == 1:
        y[b, 0, :, :] = PATCH
    else:
        y[b, 0, -2:, -2:] = PATCH


def blown(x, max_value):
    """the blow-up predicate of the kernels: NOT every |x| <= max_value, so a NaN raises it"""
    return not bool(np.all(np.abs(x) <= max_value))


def blowup_inputs(case):
    """inputs of test d (B = 5, one control step): the tame ones, and a copy with the patch on trajectory 1 and one NaN cell
    (u, mid-grid) in trajectory 3"""
    c = case_of(case)
    y0, act, prev = inputs(c, BLOWUP_B, steps=1, seed=7)
    bad = y0.copy()
    patch(bad, 1)
    bad[3, 0, c.ny // 2, c.nx // 2] = np.nan
    return y0, bad, act[0], prev


def mag(cfg, y, p):
    """oracle.keller_segel2d.f with every term replaced by its absolute value and every subtraction by an addition: the scale
    of the rounding errors of one right-hand side, per cell ([2, ny, nx])"""
    dx = cfg.dx

    def nb(a):
        return (np.concatenate([a[:, :1], a[:, :-1]], axis=1), np.concatenate([a[:, 1:], a[:, -1:]], axis=1),
                np.concatenate([a[:1, :], a[:-1, :]], axis=0), np.concatenate([a[1:, :], a[-1:, :]], axis=0))

    u, v = np.abs(y[0]), np.abs(y[1])
    uw, ue, us, un = nb(u)
    vw, ve, vs, vn = nb(v)
    ux, uy = 0.5 / dx * uw + 0.5 / dx * ue, 0.5 / dx * us + 0.5 / dx * un
    vx, vy = 0.5 / dx * vw + 0.5 / dx * ve, 0.5 / dx * vs + 0.5 / dx * vn
    lu = (uw / dx ** 2 + 2.0 / dx ** 2 * u + ue / dx ** 2) + (us / dx ** 2 + 2.0 / dx ** 2 * u + un / dx ** 2)
    lv = (vw / dx ** 2 + 2.0 / dx ** 2 * v + ve / dx ** 2) + (vs / dx ** 2 + 2.0 / dx ** 2 * v + vn / dx ** 2)
    vdot = lv + v + u + np.abs(p)
    udot = lu + u + 5.6 * ux * vx + 5.6 * uy * vy + 5.6 * u * lv + u ** 2
    return np.stack([udot, vdot])


# ------------------------------------------------------------------ the host rules, restated
def tiles(nx, ny, tsize):
    """(ntx, nty) of kseg2d_rk4_kernel: tiles of 64 columns, 64 rows in fp32 (tsize 4) and 32 in fp64 (tsize 8)"""
    ty = 64 if tsize == 4 else 32
    return -(-nx // TX), -(-ny // ty)


def grid(nx, ny, B, tsize):
    ntx, nty = tiles(nx, ny, tsize)
    return ntx * nty * B


def remapped(nx, ny, B, tsize):
    """the XCD-aware tile order is taken when the grid is a multiple of 8"""
    return grid(nx, ny, B, tsize) % 8 == 0


def remap(n):
    """logical tile of every workgroup of a grid of n (the kernel's lid): a permutation of range(n)"""
    if n % 8:
        return list(range(n))
    return [(w & 7) * (n >> 3) + (w >> 3) for w in range(n)]


def parts(nx, ny, B):
    """k2_parts without the PDEC_KSEG2D_SPLIT override: the sizes of the parts a fp32 batch is stepped in ([] = unsplit);
    three parts from 1536 fp32 tiles, two from 1024; part i takes left // (np - i) trajectories"""
    t = grid(nx, ny, B, 4)
    n = 3 if t >= 1536 else (2 if t >= 1024 else 0)
    n = min(n, 4, B)                                      # PartStreams::MAX
    if n < 2:
        return []
    out, left = [], B
    for i in range(n):
        out.append(left // (n - i))
        left -= out[-1]
    return out


def picks(case):
    """the trajectories a test compares with the oracle: all of a small batch; of a split batch the first and the last of each
    part and one inside"""
    c = case_of(case)
    ps = parts(c.nx, c.ny, c.B)
    if c.B <= 8 or not ps:
        return list(range(c.B))
    out, b0 = [], 0
    for n in ps:
        out += [b0, b0 + n // 2, b0 + n - 1]
        b0 += n
    return out


def split_patched(case):
    """test e's second run: the last trajectory of part 0, the first of part 1 and the last of the batch"""
    c = case_of(case)
    ps = parts(c.nx, c.ny, c.B)
    return [ps[0] - 1, ps[0], c.B - 1]


def nsub2_launches(K):
    """sub-steps per launch of the two-sub-step variant (PDEC_KSEG2D_NSUB2): pairs while two are left, then one"""
    out, left = [], K
    while left:
        out.append(2 if left >= 2 else 1)
        left -= out[-1]
    return out


def box_range(pos, n):
    """0-based inclusive cell range of a box centred on the 1-based position pos, clipped to n cells"""
    return max(pos - 1 - HW, 0), min(pos - 1 + HW, n - 1)


def geometry(case):
    """what a row reaches, from the table's own numbers"""
    c = case_of(case)
    Sx, Sy = len(c.sensor_x), len(c.sensor_y)
    if c.a2s is None:
        by = min(c.border, (Sy - 1) // 2)
        a2s = [iy * Sx + ix for iy in range(by, Sy - by) for ix in range(c.border, Sx - c.border)]
    else:
        a2s = [a - 1 for a in c.a2s]
    wx = [box_range(p, c.nx) for p in c.sensor_x]
    wy = [box_range(p, c.ny) for p in c.sensor_y]
    cells = lambda s: (wy[s // Sx][1] - wy[s // Sx][0] + 1) * (wx[s % Sx][1] - wx[s % Sx][0] + 1)
    side = 2 * HW + 1
    w = c.window_size // 2
    return dict(
        Sx=Sx, Sy=Sy, S=Sx * Sy, A=len(a2s), a2s=a2s, ns=2 * c.window_size ** 2 * c.temporal_steps,
        acnt=[cells(s) for s in a2s], scnt=[cells(s) for s in range(Sx * Sy)],
        clipped=any(cells(s) != side * side for s in range(Sx * Sy)),
        actuator_clipped=any(cells(s) != side * side for s in a2s),
        sensor_overlap=any(wx[i][1] >= wx[i + 1][0] for i in range(Sx - 1)) or any(wy[i][1] >= wy[i + 1][0] for i in range(Sy - 1)),
        sensor_pass2=Sx > 64, column_pass2=c.nx > 256, monotone=all(b > a for a, b in zip(a2s, a2s[1:])),
        window_wraps_x=any(s % Sx - w < 0 or s % Sx + w >= Sx for s in a2s),
        window_wraps_y=any(s // Sx - w < 0 or s // Sx + w >= Sy for s in a2s),
        window_revisits=c.window_size > min(Sx, Sy),
        last_cell_actuated=any(wx[s % Sx][1] == c.nx - 1 and wy[s // Sx][1] == c.ny - 1 for s in a2s),
        tiles={ts: tiles(c.nx, c.ny, ts) for ts in (4, 8)}, grid={ts: grid(c.nx, c.ny, c.B, ts) for ts in (4, 8)},
        remapped={ts: remapped(c.nx, c.ny, c.B, ts) for ts in (4, 8)},
        tiles_divide_8={ts: 8 % (tiles(c.nx, c.ny, ts)[0] * tiles(c.nx, c.ny, ts)[1]) == 0 for ts in (4, 8)},
        parts=parts(c.nx, c.ny, c.B),
        last_strip_only=c.nx % TX == 4, last_row_only={4: c.ny % 64 == 1, 8: c.ny % 32 == 1})
