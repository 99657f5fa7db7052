#!/usr/bin/env python3
"""Generator of the hand-written run of lean pieces of fwd_kernel<float, 16, 1, 8, 4, true> (phlash_amd/csrc/fwd_run_k16r1.inc).

Why (profiles/r05_ab_experiments.txt items 16, 19, 21; r06 item 0): the kernel runs as lone waves, one per SIMD, and a lone
wave pays an issue slot for every instruction -- a scalar bit test, a not-taken branch and a v_mov cost what a packed fma costs.
The compiler's one block body (fold_piece in fwd_kernel_body.inc) carries eight per-site test-and-branch groups, twelve v_mov that
pair a scan entry with a zero, and 64-bit address arithmetic for its four checkpoint stores, although 72-85 % of the blocks at 1 %
hets are hom in both rows of the wave.  This file owns the WHOLE run of lean pieces of a wave that holds at most two observation
rows and whose sequences fold: the piece loop with its scalar loads one piece ahead, the segment bookkeeping, the block loop, an
all-hom body without tests and a mixed body with them, the stores and the loop budget -- one asm statement under one register
plan, whose operands are the run's state (as scripts/gen_sweep_asm.py does for the sweeps; its register-plan and hazard code
is reused here).

The arithmetic is Lane<float, 16, 1>::fwd_site<false> / fwd_site_sum<false>, operation for operation: per site the chain
pre(u.*a) -- fifteen v_fma_f32, ascending, the first on a zero -- the chain suf(a) -- fifteen v_add_f32, descending, the first
on a zero; a sixteenth add at the two rescale sites hands out the sum of the entering state -- and the combine d.*a, + v.*pre,
+ b.*suf as 24 packed instructions; rescale on demand (Lane::rescale_on_demand) as one v_cmp and one branch per rescale site, its
body out of line -- and behind a block's first rescale a copy of the block's remaining sites and of the block end that books the
exponent, so that a block which does not rescale (nearly all) stores the chain's zero and touches neither eblk's register nor eb_min.  Every instruction has the operands of the compiler's, in the compiler's order, so the results are bit-identical
(tests/test_fwd_run.py).  What is gone: the pairing v_mov (the zero of a chain sits in the chain's own register file: P[0] and
S[15] are written once per run), the per-site tests of an all-hom block, the store addresses (wave-uniform base in SGPRs, four
32-bit lane offsets that never change).

The state ping-pongs between two register sets (site i reads set i % 2 and writes the other), so alpha of a block's left edge
stays in set 0 until the combine of site 1: the window in which its four 1 KB checkpoint stores are issued.

    python scripts/gen_fwd_asm.py [out.inc] [--stores=spread|clustered]   write the sequence and print the counts
    python scripts/gen_fwd_asm.py --report [--stores=...]                 only print the instructions of one trip, per kind of block

--stores=clustered (default)  all four stores at the block's top, as the C++ body issues them;  spread: 22 instructions apart over
sites 0 and 1.  Same addresses, same data, same bits -- and the same time (profiles/ab_fwd_run.txt item 4: 8.087 against 8.084 ms of
cfg2's forward phase), so the stores stay where the plan is simplest.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_sweep_asm import Gen  # noqa: E402

FBASE = 176          # first clobbered VGPR
NP = 8               # packed pairs per lane (16 states, pair h = states 2h, 2h + 1)
T = 8                # sites per block
RESCALE_SITES = (3, 7)
# positions (site, instructions of that site already issued) of the four checkpoint stores
STORES = {"spread": [(0, 10), (0, 32), (0, 54), (1, 22)], "clustered": [(0, 0), (0, 0), (0, 0), (0, 0)]}

# clobbered SGPRs
NA, NB = "s[64:67]", "s[68:71]"          # the piece requested ahead, rows A and B
CA = ["s72", "s73", "s74", "s75"]        # the current piece: the low pair is shifted down block by block
CB = ["s76", "s77", "s78", "s79"]
S_T, S_CU, S_NH, S_CA, S_CB, S_CNT, S_HALF = "s80", "s81", "s82", "s83", "s84", "s85", "s86"
S_ADR = {"A": ("s[88:89]", "s88", "s89"), "B": ("s[96:97]", "s96", "s97")}   # addresses of the two scalar loads
S_SAVE = "s[90:91]"
CKU, CKU_LO, CKU_HI = "s[92:93]", "s92", "s93"   # wave-uniform base of the block's checkpoint stores ...
EBU, EBU_LO, EBU_HI = "s[94:95]", "s94", "s95"   # ... and of its exponent store
SGPR_CLOBBERS = range(64, 98)


def build(stores="clustered"):
    g = Gen()
    g.next_free = FBASE
    # ---- operands ---------------------------------------------------------------------------------------------------------
    AOP = [f"%[a{h}]" for h in range(NP)]
    U = [f"%[u{i}]" for i in range(16)]
    PD = [f"%[pd{h}]" for h in range(NP)]
    PV = [f"%[pv{h}]" for h in range(NP)]
    PB = [f"%[pb{h}]" for h in range(NP)]
    OFF = [f"%[off{q}]" for q in range(4)]
    E, EXS, EBM, ESP, SQOFF, LDS = "%[E]", "%[exs]", "%[ebm]", "%[esp]", "%[sqoff]", "%[lds]"
    BLK, PC, BUDGET, SEGL = "%[blk]", "%[pc]", "%[budget]", "%[segl]"
    NPM1, NFULL, BLKW, SEGB = "%[npm1]", "%[nfull]", "%[blkw]", "%[segb]"
    ESPSTEP, ACT, ROWB, THR = "%[espstep]", "%[act]", "%[rowb]", "%[thr]"   # (64-bit operands used whole, and the trigger)
    # 64-bit scalars whose halves a carry chain addresses come as two 32-bit operands each
    PA, PBS = ("%[pa_lo]", "%[pa_hi]"), ("%[pb_lo]", "%[pb_hi]")
    CKSTEP, EBSTEP = ("%[ckstep_lo]", "%[ckstep_hi]"), ("%[ebstep_lo]", "%[ebstep_hi]")

    # ---- temporaries ------------------------------------------------------------------------------------------------------
    AQ = [[g.quad() for q in range(4)] for s in range(2)]        # the two state sets, quad q = states 4q .. 4q + 3
    A = [[("p", AQ[s][h // 2][1] + 2 * (h % 2)) for h in range(NP)] for s in range(2)]
    PQ = [g.quad() for q in range(4)]                            # P[i] = pre(u.*a)[i], P[0] = 0 for the whole run
    SQ = [g.quad() for q in range(4)]                            # S[i] = suf(a)[i], S[15] = 0 for the whole run
    P = [("s", PQ[0][1] + i) for i in range(16)]
    S = [("s", SQ[0][1] + i) for i in range(16)]
    PP = [("p", PQ[0][1] + 2 * h) for h in range(NP)]
    SP = [("p", SQ[0][1] + 2 * h) for h in range(NP)]
    ROWQ = [PQ[1], PQ[2], PQ[3], SQ[0]]                          # a het / missing site's emission row (the chains are dead there)
    ROW = [("p", ROWQ[h // 2][1] + 2 * (h % 2)) for h in range(NP)]
    SCP = g.pair()                                               # the rescale's factor in the low half
    SC, EX = g.lo(SCP), g.hi(SCP)
    SUM, T0, DE = g.single(), g.single(), g.single()

    def a_(s, i):
        """state i of set s"""
        return ("s", A[s][0][1] + i)

    def salu(text):
        g.emit(text, kind="salu")

    def branch(text):
        g.emit(text, kind="branch")

    # ---- prologue of the run ----------------------------------------------------------------------------------------------
    salu("s_nop 4")  # (whatever wrote the statement's scalar operands is behind us)
    for h in range(NP):
        g.mov64(A[0][h], AOP[h])
    g.emit(f"v_mov_b32_e32 {g.txt(P[0])}, 0", [P[0]], [])
    g.emit(f"v_mov_b32_e32 {g.txt(S[15])}, 0", [S[15]], [])

    def request(pc_reg, plus_one):
        """s_load of piece min(pc + plus_one, npieces - 1) of both rows into NA / NB"""
        if plus_one:
            salu(f"s_add_i32 {S_T}, {pc_reg}, 1")
            salu(f"s_min_i32 {S_T}, {S_T}, {NPM1}")
            salu(f"s_lshl_b32 {S_T}, {S_T}, 4")
        else:
            salu(f"s_lshl_b32 {S_T}, {pc_reg}, 4")
        for base, dst, (adr, adr_lo, adr_hi) in ((PA, NA, S_ADR["A"]), (PBS, NB, S_ADR["B"])):
            salu(f"s_add_u32 {adr_lo}, {base[0]}, {S_T}")
            salu(f"s_addc_u32 {adr_hi}, {base[1]}, 0")
            g.emit(f"s_load_dwordx4 {dst}, {adr}, 0x0", kind="smem")

    salu(f"s_mov_b32 {CKU_LO}, %[cku_lo]")
    salu(f"s_mov_b32 {CKU_HI}, %[cku_hi]")
    salu(f"s_mov_b32 {EBU_LO}, %[ebu_lo]")
    salu(f"s_mov_b32 {EBU_HI}, %[ebu_hi]")
    request(PC, False)
    piece_top, half_top, blk_top = g.newlabel("piece"), g.newlabel("half"), g.newlabel("top")
    mixed, latch, piece_end, done = g.newlabel("mixed"), g.newlabel("latch"), g.newlabel("pend"), g.newlabel("done")
    latch2 = g.newlabel("join")
    noseg, segdec, lean2 = g.newlabel("noseg"), g.newlabel("segdec"), g.newlabel("lean")

    # ---- one piece: land it, request the next, segment bookkeeping ---------------------------------------------------------
    g.label(piece_top)
    g.emit("s_waitcnt lgkmcnt(0)", kind="wait")
    salu(f"s_mov_b64 s[72:73], s[64:65]")
    salu(f"s_mov_b64 s[74:75], s[66:67]")
    salu(f"s_mov_b64 s[76:77], s[68:69]")
    salu(f"s_mov_b64 s[78:79], s[70:71]")
    request(PC, True)
    salu(f"s_cmp_eq_u32 {SEGB}, 0")
    branch(f"s_cbranch_scc1 {noseg}")
    salu(f"s_cmp_lg_u32 {SEGL}, 0")
    branch(f"s_cbranch_scc1 {segdec}")
    salu(f"s_and_saveexec_b64 {S_SAVE}, {ACT}")
    g.emit(f"global_store_dword {ESP}, {E}, off", [], [ESP, E], "vmem")
    salu(f"s_mov_b64 exec, {S_SAVE}")
    g.emit(f"v_lshl_add_u64 {ESP}, {ESP}, 0, {ESPSTEP}", [ESP], [ESP])
    salu(f"s_mov_b32 {SEGL}, {SEGB}")
    g.label(segdec)
    salu(f"s_add_i32 {SEGL}, {SEGL}, -8")
    g.label(noseg)
    salu(f"s_mov_b32 {S_HALF}, 0")
    g.label(half_top)
    salu(f"s_mov_b32 {S_CNT}, 8")

    cold = []

    def store(q):
        g.emit(f"global_store_dwordx4 {OFF[q]}, {g.txt(AQ[0][q])}, {CKU} nt", [], [OFF[q], AQ[0][q]], "vmem")

    def site(i, tests, behind_rescale=False):
        """behind_rescale: the copy of the block's rest that a block runs once a rescale has fired in it (out of line)"""
        cur, new = A[i % 2], A[(i + 1) % 2]
        s = i % 2
        n = [0]  # instructions of this site issued so far
        due = [q for q, (si, _) in enumerate(STORES[stores]) if si == i]

        def tick():
            for q in list(due):
                if STORES[stores][q][1] <= n[0]:
                    store(q)
                    due.remove(q)
            n[0] += 1

        # the two chains, interleaved: P[k + 1] = fma(u_k, a_k, P[k]);  S[k - 1] = a_k + S[k]
        for k in range(15):
            tick()
            g.emit(f"v_fma_f32 {g.txt(P[k + 1])}, {U[k]}, {g.txt(a_(s, k))}, {g.txt(P[k])}", [P[k + 1]], [U[k], a_(s, k), P[k]])
            tick()
            g.emit(f"v_add_f32_e32 {g.txt(S[14 - k])}, {g.txt(a_(s, 15 - k))}, {g.txt(S[15 - k])}", [S[14 - k]], [a_(s, 15 - k), S[15 - k]])
        if i in RESCALE_SITES:  # the sum of the state entering the site: the suffix chain's total
            tick()
            g.emit(f"v_add_f32_e32 {g.txt(SUM)}, {g.txt(a_(s, 0))}, {g.txt(S[0])}", [SUM], [a_(s, 0), S[0]])
        for h in range(NP):
            tick()
            g.pk_mul(new[h], PD[h], cur[h])
        for h in range(NP):
            tick()
            g.pk_fma(new[h], PV[h], PP[h], new[h])
        for h in (7, 0, 6, 1, 5, 2, 4, 3):  # (the next site's chains begin with states 0 and 15)
            tick()
            g.pk_fma(new[h], PB[h], SP[h], new[h])
        tick()
        assert not due, (i, due)
        if tests:
            lab, ret = g.newlabel(f"het{i}"), g.newlabel(f"hr{i}")
            salu(f"s_bitcmp1_b32 {S_NH}, {2 * i}")
            branch(f"s_cbranch_scc1 {lab}")
            g.label(ret)
            cold.append(("het", i, lab, ret, new))
        if i in RESCALE_SITES and behind_rescale:  # (already out of line: the body stands behind its test)
            skip = g.newlabel(f"rk{i}")
            g.emit(f"v_cmp_gt_f32_e32 vcc, {THR}, {g.txt(SUM)}", [], [SUM], "vcmp")
            branch(f"s_cbranch_vccz {skip}")
            rescale(new, first=False)
            g.label(skip)
        elif i in RESCALE_SITES:
            lab = g.newlabel(f"rs{i}")
            g.emit(f"v_cmp_gt_f32_e32 vcc, {THR}, {g.txt(SUM)}", [], [SUM], "vcmp")
            branch(f"s_cbranch_vccnz {lab}")
            cold.append(("rescale", i, lab, tests, new))

    def rescale(new, first):
        """Lane::rescale_on_demand behind its test: vcc = the lanes whose sum fell below the trigger.  DE: the block's exponent so far"""
        g.emit(f"v_frexp_exp_i32_f32_e32 {g.txt(T0)}, {g.txt(SUM)}", [T0], [SUM])
        g.emit(f"v_cndmask_b32_e32 {g.txt(EX)}, 0, {g.txt(T0)}, vcc", [EX], [T0])
        g.emit(f"v_sub_u32_e32 {g.txt(T0)}, 0, {g.txt(EX)}", [T0], [EX])
        g.emit(f"v_ldexp_f32 {g.txt(SC)}, 1.0, {g.txt(T0)}", [SC], [T0])
        for h in range(NP):
            g.emit(f"v_pk_mul_f32 {g.txt(new[h])}, {g.txt(SCP)}, {g.txt(new[h])} op_sel_hi:[0,1]", [new[h]], [SC, new[h]], "pk")
        g.emit(f"v_add_u32_e32 {g.txt(T0)}, 64, {g.txt(EX)}", [T0], [EX])        # ex - RISK_EXP_F32
        g.emit(f"v_add_u32_e32 {E}, {g.txt(EX)}, {E}", [E], [EX, E])
        if first:
            g.emit(f"v_mov_b32_e32 {g.txt(DE)}, {g.txt(EX)}", [DE], [EX])
        else:
            g.emit(f"v_add_u32_e32 {g.txt(DE)}, {g.txt(EX)}, {g.txt(DE)}", [DE], [EX, DE])
        g.emit(f"v_min_i32_e32 {EXS}, {EXS}, {g.txt(T0)}", [EXS], [EXS, T0])

    # ---- the block loop: all-hom body in line, mixed body behind the loop ---------------------------------------------------
    g.label(blk_top)
    salu(f"s_or_b32 {S_T}, {CA[0]}, {CB[0]}")
    salu(f"s_and_b32 {S_CU}, {S_T}, 0xffff")
    branch(f"s_cbranch_scc1 {mixed}")
    for i in range(T):
        site(i, False)
    g.label(latch)
    # A block that arrives here has not rescaled (one that has runs its rest out of line and joins at latch2): its exponent is the
    # zero of the prefix chain, and eb_min -- never above zero -- stays what it is.
    g.emit(f"global_store_short {SQOFF}, {g.txt(P[0])}, {EBU}", [], [SQOFF, P[0]], "vmem")
    g.label(latch2)
    salu("s_lshr_b64 s[72:73], s[72:73], 16")
    salu("s_lshr_b64 s[76:77], s[76:77], 16")
    salu(f"s_add_u32 {CKU_LO}, {CKU_LO}, {CKSTEP[0]}")
    salu(f"s_addc_u32 {CKU_HI}, {CKU_HI}, {CKSTEP[1]}")
    salu(f"s_add_u32 {EBU_LO}, {EBU_LO}, {EBSTEP[0]}")
    salu(f"s_addc_u32 {EBU_HI}, {EBU_HI}, {EBSTEP[1]}")
    salu(f"s_lshr_b32 {S_CNT}, {S_CNT}, 1")         # 8, 4, 2, 1 -> scc = 0 after the fourth block
    branch(f"s_cbranch_scc1 {blk_top}")
    # the piece's second half, or the piece's end
    salu(f"s_cmp_lg_u32 {S_HALF}, 0")
    branch(f"s_cbranch_scc1 {piece_end}")
    salu(f"s_mov_b32 {S_HALF}, 1")
    salu("s_mov_b64 s[72:73], s[74:75]")
    salu("s_mov_b64 s[76:77], s[78:79]")
    branch(f"s_branch {half_top}")
    g.label(piece_end)
    salu(f"s_add_i32 {BLK}, {BLK}, 8")
    salu(f"s_add_i32 {PC}, {PC}, 1")
    # while (lean_piece(blk) && --budget >= 0)
    salu(f"s_add_i32 {S_T}, {BLK}, 8")
    salu(f"s_cmp_gt_i32 {S_T}, {NFULL}")
    branch(f"s_cbranch_scc1 {done}")
    salu(f"s_cmp_lt_i32 {BLKW}, {BLK}")
    branch(f"s_cbranch_scc1 {lean2}")
    salu(f"s_cmp_ge_i32 {BLKW}, {S_T}")
    branch(f"s_cbranch_scc0 {done}")
    g.label(lean2)
    salu(f"s_add_i32 {BUDGET}, {BUDGET}, -1")
    salu(f"s_cmp_lt_i32 {BUDGET}, 0")
    branch(f"s_cbranch_scc0 {piece_top}")
    branch(f"s_branch {done}")

    # ---- mixed block --------------------------------------------------------------------------------------------------------
    g.label(mixed)
    salu(f"s_lshr_b32 {S_T}, {S_CU}, 1")
    salu(f"s_or_b32 {S_NH}, {S_CU}, {S_T}")      # bit 2i: site i is not hom in one of the wave's rows
    salu(f"s_and_b32 {S_CA}, {CA[0]}, 0xffff")
    salu(f"s_and_b32 {S_CB}, {CB[0]}, 0xffff")
    for i in range(T):
        site(i, True)
    branch(f"s_branch {latch}")

    # ---- cold bodies ----------------------------------------------------------------------------------------------------------
    while cold:  # (the rest of a rescaled block adds het bodies of its own)
        kind, i, lab, ret, new = cold.pop(0)
        g.label(lab)
        if kind == "het":
            # every lane multiplies by the row of its own code (a folded lane's hom row is exactly 1)
            g.emit(f"v_mov_b32_e32 {g.txt(T0)}, {S_CA}", [T0], [])
            g.emit(f"v_mov_b32_e32 {g.txt(SC)}, {S_CB}", [SC], [])
            g.emit(f"v_cndmask_b32_e64 {g.txt(T0)}, {g.txt(T0)}, {g.txt(SC)}, {ROWB}", [T0], [T0, SC])  # this lane's codes of the block
            g.emit(f"v_bfe_u32 {g.txt(T0)}, {g.txt(T0)}, {2 * i}, 2", [T0], [T0])
            g.emit(f"v_lshl_add_u32 {g.txt(T0)}, {g.txt(T0)}, 6, {LDS}", [T0], [T0, LDS])  # the row of its code in the lane's table
            for q in range(4):
                g.emit(f"ds_read_b128 {g.txt(ROWQ[q])}, {g.txt(T0)} offset:{16 * q}", [ROWQ[q]], [T0], "lds")
            g.emit("s_waitcnt lgkmcnt(0)", kind="wait")
            for h in range(NP):
                g.pk_mul(new[h], ROW[h], new[h])
            branch(f"s_branch {ret}")
        else:
            # The first rescale of a block, and with it the block's rest: the sites still to come (with their tests where the block
            # is mixed; `ret` says so), the second rescale site behind its test, and the block's end with its exponent -- so that the
            # block that does not rescale carries neither the exponent's register nor its minimum.
            tests = ret
            rescale(new, first=True)
            for j in range(i + 1, T):
                site(j, tests, behind_rescale=True)
            g.emit(f"global_store_short {SQOFF}, {g.txt(DE)}, {EBU}", [], [SQOFF, DE], "vmem")
            g.emit(f"v_min_i32_e32 {EBM}, {EBM}, {g.txt(DE)}", [EBM], [EBM, DE])
            branch(f"s_branch {latch2}")

    g.label(done)
    g.emit("s_waitcnt lgkmcnt(0)", kind="wait")  # (the piece requested ahead lands in clobbered registers: before anyone else owns them)
    for h in range(NP):
        g.mov64(AOP[h], A[0][h])
    lines, nops = g.finish()
    return lines, nops, g.next_free


def trip_counts(lines):
    """Instruction mix of one trip through the block loop, per kind of block.  all-hom: from the loop's top to its latch branch;
    mixed: the top's three instructions, the mixed body (its eight tests falling through; the cold bodies lie behind it), the latch."""
    def find(stem, start=0):
        return next(n for n in range(start, len(lines)) if lines[n].startswith(f".Lphk_{stem}_") and lines[n].endswith(":"))

    top, lat, mix = find("top"), find("latch"), find("mixed")
    lat_end = next(n for n in range(lat, len(lines)) if lines[n].startswith("s_cbranch_scc1"))
    mix_end = next(n for n in range(mix, len(lines)) if lines[n].startswith("s_branch"))
    hom = lines[top:lat_end + 1]
    mixed = lines[top:top + 4] + lines[mix:mix_end + 1] + lines[lat:lat_end + 1]
    res = {}
    for name, body in (("all-hom", hom), ("mixed", mixed)):
        ins = [ln.split()[0] for ln in body if not ln.endswith(":")]
        res[name] = {
            "total": len(ins),
            "VALU": sum(m.startswith("v_") for m in ins),
            "packed": sum(m.startswith("v_pk_") for m in ins),
            "v_fma": sum(m == "v_fma_f32" for m in ins),
            "v_add": sum(m.startswith("v_add_f32") for m in ins),
            "v_mov": sum(m.startswith("v_mov") for m in ins),
            "scalar": sum(m.startswith("s_") and not m.startswith(("s_cbranch", "s_branch", "s_nop", "s_waitcnt")) for m in ins),
            "branch": sum(m.startswith(("s_cbranch", "s_branch")) for m in ins),
            "s_nop": sum(m == "s_nop" for m in ins),
            "stores": sum(m.startswith("global_store") for m in ins),
            "loads": sum(m.startswith(("global_load", "ds_", "s_load")) for m in ins),
        }
    return res


def write(out, lines, nops, top, stores):
    ops_io = [f'[a{h}] "+v"(a[{h}])' for h in range(NP)]
    ops_io += ['[E] "+v"(E)', '[exs] "+v"(ex_slack)', '[ebm] "+v"(eb_min)', '[esp] "+v"(fr_esp)',
               '[blk] "+s"(fr_blk)', '[pc] "+s"(fr_pc)', '[budget] "+s"(fr_budget)', '[segl] "+s"(fr_segl)']
    ops_in = [f'[u{i}] "v"(lane.u[{i // 2}][{i % 2}])' for i in range(16)]
    for nm, var in (("pd", "lane.d"), ("pv", "lane.v"), ("pb", "lane.b")):
        ops_in += [f'[{nm}{h}] "v"({var}[{h}])' for h in range(NP)]
    ops_in += [f'[off{q}] "v"(fr_off[{q}])' for q in range(4)]
    ops_in += ['[sqoff] "v"(fr_sqoff)', '[lds] "v"(fr_lds)', '[pa_lo] "s"(fr_pa_lo)', '[pa_hi] "s"(fr_pa_hi)', '[pb_lo] "s"(fr_pb_lo)', '[pb_hi] "s"(fr_pb_hi)',
               '[cku_lo] "s"(fr_cku_lo)', '[cku_hi] "s"(fr_cku_hi)', '[ebu_lo] "s"(fr_ebu_lo)', '[ebu_hi] "s"(fr_ebu_hi)', '[npm1] "s"(fr_npm1)', '[nfull] "s"(fr_nfull)',
               '[blkw] "s"(fr_blkw)', '[segb] "s"(fr_segb)', '[espstep] "s"(fr_espstep)', '[ckstep_lo] "s"(fr_ckstep_lo)', '[ckstep_hi] "s"(fr_ckstep_hi)', '[ebstep_lo] "s"(fr_ebstep_lo)', '[ebstep_hi] "s"(fr_ebstep_hi)',
               '[act] "s"(fr_act)', '[rowb] "s"(fr_rowb)', '[thr] "s"(fr_thr)']
    clob = [f'"v{i}"' for i in range(FBASE, top)] + [f'"s{i}"' for i in SGPR_CLOBBERS] + ['"vcc"', '"scc"', '"memory"']
    with open(out, "w") as f:
        f.write("// GENERATED by scripts/gen_fwd_asm.py -- do not edit.  The run of lean pieces of fwd_kernel<float, 16, 1, 8, 4, true> as one asm\n"
                f"// statement ({len(lines)} lines, {nops} s_nop inserted by the generator's hazard pass, temporaries v{FBASE}..v{top - 1}, checkpoint stores {stores}).\n")
        f.write("asm volatile(\n")
        for ln in lines:
            f.write(f'    "{ln}\\n\\t"\n')
        f.write("    : " + ", ".join(ops_io) + "\n    : " + ", ".join(ops_in) + "\n    : " + ", ".join(clob) + ");\n")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    stores = "clustered"
    for a in sys.argv[1:]:
        if a.startswith("--stores="):
            stores = a.split("=", 1)[1]
    assert stores in STORES, stores
    lines, nops, top = build(stores)
    for name, c in trip_counts(lines).items():
        print(f"{name} block: " + ", ".join(f"{k} {v}" for k, v in c.items()))
    if "--report" in sys.argv[1:]:
        return
    out = args[0] if args else "phlash_amd/csrc/fwd_run_k16r1.inc"
    write(out, lines, nops, top, stores)
    print(f"wrote {out}: {len(lines)} lines, {nops} s_nop, temporaries v{FBASE}..v{top - 1}, stores {stores}")


if __name__ == "__main__":
    main()
