"""The case table of test_gpu_fused_shapes.py and a plain-Python restatement of the shape rules of the fused MFMA DDPG passes
(csrc/mlp_mfma.hip + fused3_*.hpp: 3-layer pairs, csrc/mlp_mfma2.hip + fused2_*.hpp: 2-layer pairs).  Imports neither torch nor the library, so
test_fused_shape_table.py can hold the table against the rules on a machine without a GPU.

A row: (layers, ns, actor hidden, critic hidden, Bu, grad_scale, pair, act)
  pair  the template arguments of the critic / actor pass the row must reach -- "<MT,MTA>" of ddpg_critic_fused_kernel /
        ddpg_actor_fused_kernel, "<MT,MTA,KB>" of ddpg2_critic_kernel / ddpg2_actor_kernel -- or None: the generic passes
  act   those of the acting kernel -- "<MTA>" of policy_act_fused_kernel, "<MTA,KB>" of policy_act2_kernel -- or None

Tile edges (H + 1 hidden rows in 16-row tiles; the 2-layer input rows in k-blocks of 8 and 16-row staging tiles):
  3-layer critic H 128 | 143 (MT 9), 16 | 31 (MT 2); 2-layer critic H 336 | 351 (MT 22), 128 | 143 (MT 9); actors 1 | 15 (MTA 1), 16 | 31 (2)
  3-layer ns 1 | 14 (ns + na + 1 == KXP); 2-layer ns 6 | 7 (critic K0 7 | 8: the ones row inside block 0 | first row of a block kb
  does not count), 14 | 15 (staging rows 16 | 17: nR 1 -> 2), 15 | 16 (KB 2 -> 5), 30 | 31 (nR 2 -> 3), 39 | 40 (KB 5 -> 6), 46 (48 rows)
Batch edges: Bu 1, 15, 17, 127, 129 (a wave tile is 16 columns, a workgroup 128); 63 | 64 (pdec_ddpg_update_async applies ADAM inside
the 2-layer finish launch from 64 columns on); 3-layer 256 FCOLS | 256 FCOLS + 1 (the batch-mean reward moves to a launch of its
own); 2-layer above 256 chunks of 128 columns, where grid2_of deals tpw = ceil(nt / grid) tiles per workgroup (grid2_rule below):
  Bu = 32 789: nt = 2050 tiles, 257 chunks -> grid 256, tpw = 9 (every workgroup's second chunk is ONE tile), 228 workgroups, the last
               with 7 tiles, the last tile with 5 columns
  Bu = 32 835: nt = 2053, tpw = 9, 229 workgroups, the last with ONE tile of 3 columns
  Bu = 65 536: nt = 4096, 512 chunks -> grid 256, tpw = 16: two full chunks per workgroup, every tile full
(test_fused_shape_table.py asserts these figures from grid2_rule.)"""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "distributedconvrl-pde-control_amd", "csrc")

CASES = {
    # ---- 3-layer pairs [ns, h, h, 1] / [ns + 1, H, H, 1]
    "l3_ns1_a16_c16_bu1": (3, 1, 16, 16, 1, 1.0, "<2,2>", "<2>"),
    "l3_ns3_a16_c128_bu15": (3, 3, 16, 128, 15, 0.5, "<9,2>", "<2>"),
    "l3_ns14_a31_c31_bu17": (3, 14, 31, 31, 17, 1.0, "<2,2>", "<2>"),
    "l3_ns2_a15_c31_bu127": (3, 2, 15, 31, 127, 0.25, "<2,1>", "<1>"),
    "l3_ns7_a16_c143_bu129": (3, 7, 16, 143, 129, 1.0, "<9,2>", "<2>"),
    "l3_ns5_a31_c128_bu63": (3, 5, 31, 128, 63, 1.0, "<9,2>", "<2>"),
    "l3_ns1_a1_c143_bu64": (3, 1, 1, 143, 64, 1.0, "<9,1>", "<1>"),
    "l3_ns14_a15_c143_bu1000": (3, 14, 15, 143, 1000, 0.5, "<9,1>", "<1>"),         # the corner of the family
    "l3_ns3_a1_c16_bu32768": (3, 3, 1, 16, 32768, 1.0, "<2,1>", "<1>"),             # 256 FCOLS: every workgroup sums r itself
    "l3_ns3_a16_c143_bu32769": (3, 3, 16, 143, 32769, 1.0, "<9,2>", "<2>"),         # 256 FCOLS + 1: the mean is a launch of its own
    # ---- 2-layer pairs [ns, h, 1] / [ns + 1, H, 1]
    "l2_ns6_a16_c336_bu1": (2, 6, 16, 336, 1, 1.0, "<22,2,2>", "<2,2>"),
    "l2_ns7_a1_c351_bu15": (2, 7, 1, 351, 15, 0.5, "<22,1,2>", "<1,2>"),
    "l2_ns14_a15_c128_bu17": (2, 14, 15, 128, 17, 1.0, "<9,1,2>", "<1,2>"),
    "l2_ns15_a31_c143_bu127": (2, 15, 31, 143, 127, 1.0, "<9,2,2>", "<2,2>"),
    "l2_ns16_a16_c143_bu129": (2, 16, 16, 143, 129, 0.25, "<9,2,5>", "<2,2>"),      # critic 3 k-blocks, actor 2
    "l2_ns30_a15_c351_bu63": (2, 30, 15, 351, 63, 1.0, "<22,1,5>", "<1,5>"),
    "l2_ns31_a1_c128_bu64": (2, 31, 1, 128, 64, 1.0, "<9,1,5>", "<1,5>"),
    "l2_ns39_a31_c336_bu300": (2, 39, 31, 336, 300, 1.0, "<22,2,5>", "<2,5>"),
    "l2_ns40_a15_c336_bu1500": (2, 40, 15, 336, 1500, 0.5, "<22,1,6>", "<1,5>"),    # critic 6 k-blocks, actor 5
    "l2_ns41_a16_c143_bu777": (2, 41, 16, 143, 777, 1.0, "<9,2,6>", "<2,6>"),
    "l2_ns46_a1_c128_bu32835": (2, 46, 1, 128, 32835, 1.0, "<9,1,6>", "<1,6>"),     # the last workgroup owns one tile of 3 columns
    "l2_ns46_a31_c351_bu32789": (2, 46, 31, 351, 32789, 1.0, "<22,2,6>", "<2,6>"),  # the corner, just above the switch of grid2_of
    "l2_ns46_a31_c351_bu65536": (2, 46, 31, 351, 65536, 0.5, "<22,2,6>", "<2,6>"),  # the corner, two full chunks per workgroup
    # ---- one step outside each predicate: the generic fp32 passes
    "o3_c127": (3, 3, 16, 127, 200, 1.0, None, "<2>"),
    "o3_c144": (3, 3, 16, 144, 200, 0.5, None, "<2>"),
    "o3_c32": (3, 3, 16, 32, 200, 1.0, None, "<2>"),
    "o3_a32": (3, 3, 32, 140, 200, 1.0, None, None),
    "o3_ns15": (3, 15, 16, 140, 200, 1.0, None, "<2>"),       # (a 15-row state still fits the actor's own image: acting stays fused)
    "o2_c335": (2, 12, 20, 335, 200, 1.0, None, "<2,2>"),
    "o2_c352": (2, 12, 20, 352, 200, 0.5, None, "<2,2>"),
    "o2_c127": (2, 12, 20, 127, 200, 1.0, None, "<2,2>"),
    "o2_c144": (2, 12, 20, 144, 200, 1.0, None, "<2,2>"),
    "o2_a32": (2, 12, 32, 340, 200, 1.0, None, None),
    "o2_ns47": (2, 47, 20, 340, 200, 1.0, None, "<2,6>"),     # (47 rows fit the acting kernel's 6 k-blocks: acting stays fused)
}
FUSED = [k for k, v in CASES.items() if v[6] is not None]
OUTSIDE = [k for k, v in CASES.items() if v[6] is None]
ACT_COLS = 300          # states of the acting check: above the 256 columns from which the 2-layer acting kernel serves


def kernel_names(case):
    """(critic pass, actor pass, acting kernel) names as pdec_debug_batched_update_route reports them; None: not fused"""
    layers, _, _, _, _, _, pair, act = CASES[case]
    crit, actor, acting = (("ddpg_critic_fused_kernel", "ddpg_actor_fused_kernel", "policy_act_fused_kernel") if layers == 3 else
                           ("ddpg2_critic_kernel", "ddpg2_actor_kernel", "policy_act2_kernel"))
    return (crit + pair if pair else None, actor + pair if pair else None, acting + act if act else None)


def dims_of(case):
    """(actor dims, critic dims) of a row; activations relu ... relu, tanh | identity"""
    layers, ns, ha, hc = CASES[case][:4]
    return ([ns] + [ha] * (layers - 1) + [1], [ns + 1] + [hc] * (layers - 1) + [1])


# ------------------------------------------------------------------ the rules, restated
def read_constants(csrc=CSRC):
    """constants and instantiation lists of the dispatch, read out of the sources"""
    m3 = open(os.path.join(csrc, "mlp_mfma.hip")).read()
    m2 = open(os.path.join(csrc, "mlp_mfma2.hip")).read()
    blocks = open(os.path.join(csrc, "mfma_blocks.hpp")).read()
    layers2 = open(os.path.join(csrc, "fused2_layers.hpp")).read()

    def define(src, name):
        return int(re.search(rf"^#define {name} (\d+)\b", src, flags=re.M).group(1))

    def xlist(src, name):
        body = re.search(rf"^#define {name}\([XY]\)(.*)$", src, flags=re.M).group(1)
        return [tuple(int(v) for v in t.split(",")) for t in re.findall(r"[XY]\(([\d, ]+)\)", body)]
    k = {"KXP": define(m3, "KXP"), "K2MAX": define(m2, "K2MAX"), "FCOLS": define(blocks, "FCOLS"), "CPWMAX": define(m2, "CPWMAX"),
         "T3": xlist(m3, "FUSED3_TILES"), "A3": [t[0] for t in xlist(m3, "FUSED3_ACT_TILES")],
         "T2": xlist(m2, "FUSED2_TILES"), "A2": [t[0] for t in xlist(m2, "FUSED2_ACT_TILES")],
         "KB2": [t[0] for t in xlist(m2, "FUSED2_KBS")]}
    k["ACT2_MIN_COLS"] = int(re.search(r"bool fused2_act_supported\(.*?cols < (\d+)\)", m2, flags=re.S).group(1))
    k["APPLY2_MIN_BU"] = define(m2, "FUSED2_APPLY_MIN_BU")
    k["ACT3_MAX_H"] = define(m3, "FUSED3_ACT_MAX_H")
    k["LDP"], k["LDQ"] = define(blocks, "LDP"), define(layers2, "LDQ")      # leading dims of the 64- / 32-column staging images
    return k


def tiles_of(H):
    return -(-(H + 1) // 16)        # ceil((H + 1) / 16): the hidden units and the bias / output row


def rule(layers, ns, ha, hc, k, cols=ACT_COLS):
    """(pair, act) template-argument strings the dispatch must pick for relu/tanh actors [ns, ha (, ha), 1] and relu/identity
    critics [ns + 1, hc (, hc), 1] in fp32 on one stream, None where the predicates refuse"""
    mt, mta = tiles_of(hc), tiles_of(ha)
    if layers == 3:
        pair = f"<{mt},{mta}>" if ns + 1 + 1 <= k["KXP"] and (mt, mta) in k["T3"] else None
        # a single net's image: K0 + 1 <= KXP rows (fused_net_supported), hidden width up to ACT3_MAX_H
        act = f"<{mta}>" if ns + 1 <= k["KXP"] and mta in k["A3"] and ha <= k["ACT3_MAX_H"] else None
        return pair, act

    def kb_of(K0):
        return next((v for v in k["KB2"] if -(-K0 // 8) <= v), None)
    assert max(k["KB2"]) == k["K2MAX"]
    pair = None
    if ns + 2 <= 8 * k["K2MAX"] and (mt, mta) in k["T2"]:     # the critic's ns + 1 inputs and the ones row
        pair = f"<{mt},{mta},{kb_of(ns + 1)}>"
    act = f"<{mta},{kb_of(ns)}>" if ns <= 8 * k["K2MAX"] and mta in k["A2"] and cols >= k["ACT2_MIN_COLS"] else None
    return pair, act


def all_names(k):
    """every (critic pass, actor pass) pair and every acting kernel the dispatch can produce"""
    pairs = {("ddpg_critic_fused_kernel<%d,%d>" % t, "ddpg_actor_fused_kernel<%d,%d>" % t) for t in k["T3"]}
    pairs |= {("ddpg2_critic_kernel<%d,%d,%d>" % (mt, mta, kb), "ddpg2_actor_kernel<%d,%d,%d>" % (mt, mta, kb))
              for mt, mta in k["T2"] for kb in k["KB2"]}
    acts = {"policy_act_fused_kernel<%d>" % a for a in k["A3"]} | {"policy_act2_kernel<%d,%d>" % (a, kb) for a in k["A2"] for kb in k["KB2"]}
    return pairs, acts


def grid2_rule(Bu, k):
    """grid2_of: (workgroups, tiles per workgroup, tiles of the last workgroup, columns of the last tile)"""
    nt = -(-Bu // 16)
    nchunk = -(-nt // 8)
    if nchunk <= 256:
        grid, tpw = nchunk, 8
    else:
        g0 = max(256, -(-nchunk // k["CPWMAX"]))
        tpw = -(-nt // g0)
        grid = -(-nt // tpw)
    return grid, tpw, nt - (grid - 1) * tpw, Bu - 16 * (nt - 1)


def lds2_rule(ns, ha, hc, k):
    """(critic pass, actor pass, acting kernel) dynamic LDS bytes of a 2-layer pair [ns, ha, 1] / [ns + 1, hc, 1]: the byte counts
    of lds2_bytes / act2_lds as they stood before the layouts moved into Critic2Lds / Actor2Lds / Act2Lds (fused2_*.hpp), restated
    so that a drifted layout fails here.  img: a weight image [HP][8 KB + 4] with b1 [HP], w2 [HP], b2 [4].  nR: 16-row staging tiles
    of the inputs and the ones row, nr_of(K0) = (K0 + 1 + 15) // 16 -- 1 up to ns = 14 and 2 from ns = 15 on for the critic
    (K0 = ns + 1), one row later for the actor (K0 = ns), the edges the table's head comment names.  KB of both passes comes from
    the critic's ns + 1 rows, the acting kernel's from the actor's ns."""
    def kb_of(K0):
        return next(v for v in k["KB2"] if -(-K0 // 8) <= v)

    def img(HP, KB):
        return HP * (8 * KB + 4) + 2 * HP + 4
    HP, HPa, KB = 16 * tiles_of(hc), 16 * tiles_of(ha), kb_of(ns + 1)
    nR, nRa = (ns + 1 + 1 + 15) // 16, (ns + 1 + 15) // 16
    critic = img(HP, KB) + max(HP * k["LDQ"] + 16 * nR * k["LDQ"], 8 * HP) + img(HPa, KB) + HP
    actor = img(HP, KB) + img(HPa, KB) + HPa * k["LDP"] + 16 * nRa * k["LDP"] + 8 * HPa + HPa + 8
    return 4 * critic, 4 * actor, 4 * img(HPa, kb_of(ns))
