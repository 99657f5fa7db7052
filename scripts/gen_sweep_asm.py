#!/usr/bin/env python3
"""Generator of the hand-written block-run loop of the K = 16, R = 2 float32 sweeps (phlash_amd/csrc/sweep_run_k16r2.inc).

Why (profiles/r06_ab_experiments.txt items 0, 6): a wave of the sweeps pays an issue slot for every instruction, scalar tests and
not-taken branches included.  The C++ block body needs sixteen test-and-branch pairs per 8-site block (is site i hom in every
lane?) although 72-82 % of the blocks at 1 % hets are hom throughout, and every attempt to give such blocks a copy of the body
without the tests -- as a second C++ instance (rounds 4, 5), as grouped tests, as an inline-asm block beside the C++ block
(round 6) -- lost to the register allocator's copies at the join of the two bodies.  This file therefore owns the WHOLE run of
hot blocks: the loop, the prefetch of checkpoints / block exponents / observation words, the block's masks, an all-hom body
without tests and a mixed body with them, under ONE register plan, as one asm statement whose operands are the run's state.

The arithmetic is the C++ body's, operation for operation (psmc_kernels.hip, bwd_kernel, PHK_HET_REGS body; Lane::scans,
scans_adj, suffix_vw, beta_prev, carry with the SPLIT layout at R = 2): every fma / mul / add whose result the C++ source
uses is one instruction here with the same operands in the same order, so the results are bit-identical
(tests/test_asm_run_default.py, tests/test_hip_parity.py::test_asm_block_run_equals_the_cxx_body).  What is NOT repeated is
suf(v.*w) of a site where the forward pass can still find the beta pass's copy in registers (the same instructions on the same
inputs: the same bits): seven of the eight sites of an all-hom block (six in registers, one in the thread's LDS slice), three of a
mixed one (see SAVED_HOM / LDS_KEPT / SAVED_MIXED in build()).  Nor are the adds of a zero: where the C++ source adds a carry or a
first term to a zero-initialised scan entry (svw3 = 0 + cv; 0 + a3; the last entries of pre, suf and svw), `Gen.seed()` hands out the
source register instead of `v_pk_add_f32 d, x, 0`.  Every such x is a product or a sum of non-negative numbers -- never -0 -- and
the kernels keep float32 denormals, so x + 0 has the bits of x.  All of them went (per site one in the beta pass -- its carry lands
where svw3 was, the chain's total in a register of the site's result that is dead until then -- and three in the forward pass, four
where the site's vector is computed again).  Kept: none.  `seed(keep=True)` still emits the add, for an entry that would be overwritten
in place while its source must survive, and nothing needs it: the one chain that is updated in place and starts from such a seed
(suf(a): Y0 = a3, then Y0 + ca) reads a3 and writes the chain's own register.

    python scripts/gen_sweep_asm.py [out.inc]     write the sequence (the Makefile's rule) and print the counts below
    python scripts/gen_sweep_asm.py --report      only print, per kind of block, the instructions of one trip through the loop

Register plan (physical VGPRs are clobbers of the statement; the state's registers are its operands, chosen by the compiler):
    v[TBASE ...]   R[j][h], j = 0..7: the block's w vectors / the beta chain (w_j lives in R[j+1], the incoming beta -- an
                   operand -- is R[8]; beta travels from block to block in R[0]);  forward-pass temporaries: A (the checkpoint
                   state; later states live in the Z chain and in consumed w vectors), the three scan chains X (prefix of
                   u.*a), Y (suffix of a), Z (suffix of v.*w), lane totals, carries;  the prefetched checkpoint (two quads),
                   codes, scale, addresses;  and the registers that keep a site's suf(v.*w) from one pass to the other.
Hazards are kept by construction: `emit()` records the registers every instruction defines and uses, and `finish()` looks for
the places where (a) a packed-float32 instruction's result would be read by the very next instruction, or a packed instruction
would read a result of the very next-to-last one (one wait state, r05 item 19), (b) a DPP or readlane operand was written less
than three instructions earlier (two wait states).  There it first tries to pull up a later instruction of the same straight-line
stretch that depends on nothing it passes (`hoist()`: plain vector arithmetic only) and inserts an s_nop only if there is none;
as generated, neither kind of block has one left.
"""
import sys

TBASE = 118          # first clobbered VGPR
NP = 4               # packed pairs per lane (8 states)
T = 8                # sites per block


class Gen:
    def __init__(self):
        self.ins = []       # (text, defs, uses, kind)
        self.next_free = TBASE
        self.labels = 0
        self.seeds_aliased = 0  # scan seeds read from their source register instead of through an x + 0 (seed())

    # ---- register helpers ------------------------------------------------------------------------------------------------
    def pair(self):
        if self.next_free % 2:
            self.next_free += 1
        r = self.next_free
        self.next_free += 2
        assert self.next_free <= 256, "out of temporaries"
        return ("p", r)

    def single(self):
        r = self.next_free
        self.next_free += 1
        assert self.next_free <= 256
        return ("s", r)

    def quad(self):
        while self.next_free % 4:
            self.next_free += 1
        r = self.next_free
        self.next_free += 4
        assert self.next_free <= 256
        return ("q", r)

    @staticmethod
    def txt(r):
        """assembly text of a register object: physical pair / single / quad, or an operand placeholder"""
        if isinstance(r, str):
            return r
        k, n = r[0], r[1]
        if k == "p":
            return f"v[{n}:{n + 1}]"
        if k == "q":
            return f"v[{n}:{n + 3}]"
        if k == "s":
            return f"v{n}"
        raise ValueError(r)

    @staticmethod
    def regs(r):
        """set of register ids (ints for physical VGPRs, strings for operands) an object covers"""
        if isinstance(r, str):
            return {r}
        k, n = r[0], r[1]
        return set(range(n, n + {"p": 2, "q": 4, "s": 1}[k]))

    @staticmethod
    def lo(p):
        assert p[0] == "p"
        return ("s", p[1])

    @staticmethod
    def hi(p):
        assert p[0] == "p"
        return ("s", p[1] + 1)

    def emit(self, text, defs=(), uses=(), kind="valu"):
        d, u = set(), set()
        for r in defs:
            d |= self.regs(r)
        for r in uses:
            u |= self.regs(r)
        self.ins.append([text, d, u, kind])

    def label(self, name):
        self.ins.append([name + ":", set(), set(), "label"])

    def newlabel(self, stem):
        self.labels += 1
        return f".Lphk_{stem}_{self.labels}_%="

    # ---- instruction helpers (packed float32 unless said otherwise) ------------------------------------------------------
    def pk_fma(self, d, a, b, c):
        ct = "0" if c is None else self.txt(c)
        mod = " op_sel_hi:[1,1,0]" if c is None else ""
        self.emit(f"v_pk_fma_f32 {self.txt(d)}, {self.txt(a)}, {self.txt(b)}, {ct}{mod}", [d], [a, b] + ([] if c is None else [c]), "pk")

    def pk_mul(self, d, a, b):
        self.emit(f"v_pk_mul_f32 {self.txt(d)}, {self.txt(a)}, {self.txt(b)}", [d], [a, b], "pk")

    def pk_add(self, d, a, b):
        if b is None:  # x + 0 (the C++ source adds the carry to a zero-initialised scan entry)
            self.emit(f"v_pk_add_f32 {self.txt(d)}, {self.txt(a)}, 0 op_sel_hi:[1,0]", [d], [a], "pk")
        else:
            self.emit(f"v_pk_add_f32 {self.txt(d)}, {self.txt(a)}, {self.txt(b)}", [d], [a, b], "pk")

    def seed(self, d, x, keep=False):
        """The entry of a scan that the C++ source writes as 0 + x (a carry, or the first term, added to a zero-initialised entry).
        Returns the register to read for it: x itself -- every x here is a product or a sum of non-negative numbers, never -0,
        and the kernels run with float32 denormals on, so x + 0 has the bits of x and the add is not emitted -- or, with `keep`,
        d after `v_pk_add_f32 d, x, 0` (for an entry that is later overwritten in place while x must survive)."""
        if keep:
            self.pk_add(d, x, None)
            return d
        self.seeds_aliased += 1
        return x

    def lane_total(self, d, x):
        """(x.lo + x.hi, x.hi + x.lo)"""
        self.emit(f"v_pk_add_f32 {self.txt(d)}, {self.txt(x)}, {self.txt(x)} op_sel:[0,1] op_sel_hi:[1,0]", [d], [x], "pk")

    def carry(self, dst, lt, tot, mask, prefix):
        """Lane::carry at R = 2.  prefix: c = row_shr:1(lane total) & upm1, r = (c, c + tot.lo);  suffix: c = row_shl:1(...) & dnm1,
        r = (c + tot.hi, c).  lt: pair holding the lane total in its low half.  (A bit mask, not a multiply by 0 / 1: the lane read
        belongs to another sequence at the group's edge, and its inf or NaN times 0 would be NaN here: Group in psmc_kernels.hip.)"""
        if prefix:
            self.emit(f"v_and_b32_dpp {self.txt(self.lo(dst))}, {self.txt(self.lo(lt))}, {self.txt(mask)} row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1",
                      [self.lo(dst)], [self.lo(lt), mask], "dpp")
            self.emit(f"v_add_f32_e32 {self.txt(self.hi(dst))}, {self.txt(self.lo(tot))}, {self.txt(self.lo(dst))}", [self.hi(dst)], [self.lo(tot), self.lo(dst)])
        else:
            self.emit(f"v_and_b32_dpp {self.txt(self.hi(dst))}, {self.txt(self.lo(lt))}, {self.txt(mask)} row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1",
                      [self.hi(dst)], [self.lo(lt), mask], "dpp")
            self.emit(f"v_add_f32_e32 {self.txt(self.lo(dst))}, {self.txt(self.hi(tot))}, {self.txt(self.hi(dst))}", [self.lo(dst)], [self.hi(tot), self.hi(dst)])

    def mov64(self, d, s):
        self.emit(f"v_mov_b64_e32 {self.txt(d)}, {self.txt(s)}", [d], [s])

    # ---- finishing: hazards ----------------------------------------------------------------------------------------------
    @staticmethod
    def gap_needed(hist, u, kind):
        """wait states an instruction of `kind` that reads `u` needs after the instructions of `hist` (most recent last)"""
        need = 0
        if kind in ("valu", "pk", "dpp", "lane", "vmem_addr", "lds"):
            for back, (pd, pk) in enumerate(reversed(hist[-3:])):  # back = 0: previous instruction
                if not (pd & u):
                    continue
                if kind in ("dpp", "lane"):
                    need = max(need, 2 - back)
                elif pk == "pk" or kind == "pk":
                    need = max(need, 1 - back)
        return need

    HOIST_WINDOW = 24  # how far ahead finish() looks for an instruction to put where an s_nop would go

    def hoist(self, k, hist):
        """Index of a later instruction that may run where instruction k would need a wait state, or None.  Only plain vector
        arithmetic moves, and only over plain vector arithmetic (every register these read or write is on record; nothing that
        touches vcc, exec, memory or a scalar register is moved or crossed), and only if it depends on nothing it passes --
        no register of its own is read or written there, none it reads is written there: the values are the same, bit for bit --
        and needs no wait state itself."""
        for j in range(k + 1, min(k + 1 + self.HOIST_WINDOW, len(self.ins))):
            passed = self.ins[j - 1]
            if passed[3] not in ("valu", "pk", "dpp") or "vcc" in passed[0]:
                return None
            text, d, u, kind = self.ins[j]
            if kind not in ("valu", "pk") or "vcc" in text:
                continue
            if any((d & (pd | pu)) or (u & pd) for _, pd, pu, _ in self.ins[k:j]):
                continue
            if self.gap_needed(hist, u, kind) > 0:
                continue
            return j
        return None

    def finish(self):
        out = []   # final instruction list
        hist = []  # (defs, kind) of the last real instructions, most recent last ("nop" entries have empty defs)
        nops = 0
        k = 0
        while k < len(self.ins):
            text, d, u, kind = self.ins[k]
            if kind == "label":
                out.append(text)
                hist = []  # a join: be conservative, treat as fresh (the predecessor's last instructions are unknown)
                # conservative: after a label require the generic gaps again by assuming a packed write of everything -> handled by
                # emitting an s_nop 1 at labels that are branch targets (cheap: labels are block / run boundaries or cold paths)
                k += 1
                continue
            need = self.gap_needed(hist, u, kind)
            if need > 0:
                j = self.hoist(k, hist)
                if j is not None:  # an independent instruction of the same straight-line stretch takes the wait state's place
                    self.ins.insert(k, self.ins.pop(j))
                    continue
            k += 1
            if need > 0:
                out.append(f"s_nop {need - 1}")
                nops += 1
                for _ in range(need):
                    hist.append((set(), "nop"))
            out.append(text)
            if kind in ("branch",):
                hist = []
            else:
                hist.append((d if kind in ("valu", "pk", "dpp", "lane") else set(), kind))
        return out, nops


def build():
    g = Gen()
    # ---- operands of the asm statement (placeholders) -------------------------------------------------------------------
    B = [f"%[b{h}]" for h in range(NP)]          # beta (in / out)
    GB = [f"%[gb{h}]" for h in range(NP)]
    GD = [f"%[gd{h}]" for h in range(NP)]
    GU = [f"%[gu{h}]" for h in range(NP)]
    GV = [f"%[gv{h}]" for h in range(NP)]
    G1 = [f"%[g1{h}]" for h in range(NP)]
    Pb = [f"%[pb{h}]" for h in range(NP)]
    Pd = [f"%[pd{h}]" for h in range(NP)]
    Pu = [f"%[pu{h}]" for h in range(NP)]
    Pv = [f"%[pv{h}]" for h in range(NP)]
    RH = [f"%[rh{h}]" for h in range(NP)]
    UP1, DN1 = "%[up1]", "%[dn1]"
    AN = [f"%[an{i}]" for i in range(8)]         # prefetched checkpoint (floats, in / out)
    WCUR, WPREV, ENEXT = "%[wcur]", "%[wprev]", "%[enext]"
    CKQ, EBQ, WORDS, LDS = "%[ckq]", "%[ebq]", "%[words]", "%[lds]"
    BLK, WIDX, STOP, BLKLO = "%[blk]", "%[widx]", "%[stop]", "%[blklo]"
    CKSTEP, EBSTEP, CKPIECE = "%[ckstep]", "%[ebstep]", "%[ckpiece]"  # 64-bit SGPR pairs: -ck_step bytes, -eb step bytes, +piece distance bytes

    # ---- temporaries ----------------------------------------------------------------------------------------------------
    CKQ2 = g.pair()                                           # (first: everything below then starts on a multiple of four)
    R = [[g.pair() for h in range(NP)] for j in range(T)]   # R[j]: beta after site j's step = w of site j - 1 ... (see below)
    assert R[0][0][1] % 4 == 0                                # (an R[j] is two quads: parked by two 16-byte LDS accesses)
    A = [g.pair() for h in range(NP)]
    Tt = [g.pair() for h in range(NP)]
    # the scan chains as quads (so that the cold missing-site bodies can land their 16-byte LDS rows in them: the chains are dead there)
    XQ, YQ, ZQ = [g.quad(), g.quad()], [g.quad(), g.quad()], [g.quad(), g.quad()]
    XC = [("p", XQ[h // 2][1] + 2 * (h % 2)) for h in range(NP)]
    YC = [("p", YQ[h // 2][1] + 2 * (h % 2)) for h in range(NP)]
    ZC = [("p", ZQ[h // 2][1] + 2 * (h % 2)) for h in range(NP)]
    LTX, LTY, LTZ = g.pair(), g.pair(), g.pair()
    CX, CY, CZ = g.pair(), g.pair(), g.pair()
    PQ0, PQ1 = g.quad(), g.quad()                            # checkpoint pieces: states 0..3 / 4..7 of the lane
    ADDR = g.pair()
    FXP = g.pair()                                            # the block's scale 2^-e in the low half (read as a pair by v_pk_mul)
    FX = g.lo(FXP)
    # the scalars of enter() and of the cold bodies, as halves of pairs: an all-hom block has no use for them once it is entered, and
    # its body keeps a site's suf(v.*w) in the four pairs (SAVED sets, below)
    TAIL = [g.pair() for _ in range(4)]
    CODES, TMP, CC, LADDR = g.lo(TAIL[0]), g.hi(TAIL[0]), g.lo(TAIL[1]), g.hi(TAIL[1])
    ER0, ER1, GR0, GR1 = XQ[0], XQ[1], YQ[0], YQ[1]            # missing-site path: emission row and mass row halves (dead chains)
    S_T0, S_W, S_SH, S_A, S_B, S_U, S_NH, S_NM, S_TMP = "s88", "s89", "s90", "s91", "s92", "s93", "s94", "s95", "s96"
    S_SAVE = "s[98:99]"
    S_OFF = "s[86:87]"

    W = lambda i: (B if i == T - 1 else R[i + 1])  # w of site i lives where beta stood when the site was entered
    # beta after site i's step goes to R[i]; the block's output R[0] is the next block's input (scaled into B at its top)

    def quad_lane(q, i):
        return ("s", q[1] + i)

    # ---- prologue of the run: checkpoint prefetch registers, second piece pointer -----------------------------------------
    for i in range(4):
        g.emit(f"v_mov_b32_e32 {g.txt(quad_lane(PQ0, i))}, {AN[i]}", [quad_lane(PQ0, i)], [AN[i]])
        g.emit(f"v_mov_b32_e32 {g.txt(quad_lane(PQ1, i))}, {AN[4 + i]}", [quad_lane(PQ1, i)], [AN[4 + i]])
    g.emit(f"v_lshl_add_u64 {g.txt(CKQ2)}, {CKQ}, 0, {CKPIECE}", [CKQ2], [CKQ], "valu")
    # beta travels from block to block in R[0], where the beta pass leaves it: the scale at a block's top moves it to B (= w of the
    # block's last site) on the way, and only the run's two ends copy
    for h in range(NP):
        g.mov64(R[0][h], B[h])

    top = g.newlabel("top")
    g.label(top)
    # ---- enter(): words, checkpoint, exponent ---------------------------------------------------------------------------
    g.emit("s_waitcnt vmcnt(0)", kind="wait")
    g.emit(f"s_lshl_b32 {S_T0}, {BLK}, 3", kind="salu")
    g.emit(f"s_lshr_b32 {S_W}, {S_T0}, 4", kind="salu")
    g.emit(f"s_cmp_lg_u32 {S_W}, {WIDX}", kind="salu")
    same = g.newlabel("sameword")
    g.emit(f"s_cbranch_scc0 {same}", kind="branch")
    g.emit(f"s_mov_b32 {WIDX}, {S_W}", kind="salu")
    g.emit(f"v_mov_b32_e32 {WCUR}, {WPREV}", [WCUR], [WPREV])
    g.emit(f"s_sub_i32 {S_TMP}, {S_W}, 1", kind="salu")
    g.emit(f"s_max_i32 {S_TMP}, {S_TMP}, 0", kind="salu")
    g.emit(f"s_lshl_b32 s86, {S_TMP}, 2", kind="salu")
    g.emit("s_mov_b32 s87, 0", kind="salu")
    g.emit(f"v_lshl_add_u64 {g.txt(ADDR)}, {WORDS}, 0, {S_OFF}", [ADDR], [WORDS])
    g.emit("s_nop 0", kind="salu")
    g.emit(f"global_load_dword {WPREV}, {g.txt(ADDR)}, off", [WPREV], [ADDR], "vmem")
    g.label(same)
    # codes = the block's sixteen bits of wcur, from bit 2 * (t0 & 15) on; t0 & 15 is 0 or 8.  (Read by the masks far below: the
    # two lane reads there then need no wait state.  wcur, if just stepped, was written three instructions back by a plain move.)
    g.emit(f"s_and_b32 {S_SH}, {S_T0}, 8", kind="salu")
    g.emit(f"s_lshl_b32 {S_SH}, {S_SH}, 1", kind="salu")
    g.emit(f"v_bfe_u32 {g.txt(CODES)}, {WCUR}, {S_SH}, 16", [CODES], [WCUR])
    # al0: state i of the lane -> pair i % 4, half i / 4
    for h in range(NP):
        g.emit(f"v_mov_b32_e32 {g.txt(g.lo(A[h]))}, {g.txt(quad_lane(PQ0, h))}", [g.lo(A[h])], [quad_lane(PQ0, h)])
        g.emit(f"v_mov_b32_e32 {g.txt(g.hi(A[h]))}, {g.txt(quad_lane(PQ1, h))}", [g.hi(A[h])], [quad_lane(PQ1, h)])
    # beta *= 2^-e_fwd (e_fwd = e_next as it stands)
    g.emit(f"v_sub_u32_e32 {g.txt(TMP)}, 0, {ENEXT}", [TMP], [ENEXT])
    g.emit(f"v_ldexp_f32 {g.txt(FX)}, 1.0, {g.txt(TMP)}", [FX], [TMP])
    # prefetch the previous block's checkpoint and exponent (blk > blk_lo), step the pointers
    nopf = g.newlabel("nopf")
    g.emit(f"s_cmp_gt_i32 {BLK}, {BLKLO}", kind="salu")
    g.emit(f"s_cbranch_scc0 {nopf}", kind="branch")
    g.emit(f"global_load_dwordx4 {g.txt(PQ0)}, {CKQ}, off", [PQ0], [CKQ], "vmem")
    g.emit(f"global_load_dwordx4 {g.txt(PQ1)}, {g.txt(CKQ2)}, off", [PQ1], [CKQ2], "vmem")
    g.emit(f"global_load_sshort {ENEXT}, {EBQ}, off", [ENEXT], [EBQ], "vmem")
    g.emit(f"v_lshl_add_u64 {CKQ}, {CKQ}, 0, {CKSTEP}", [CKQ], [CKQ])
    g.emit(f"v_lshl_add_u64 {g.txt(CKQ2)}, {g.txt(CKQ2)}, 0, {CKSTEP}", [CKQ2], [CKQ2])
    g.emit(f"v_lshl_add_u64 {EBQ}, {EBQ}, 0, {EBSTEP}", [EBQ], [EBQ])
    g.label(nopf)
    # scale: beta = fx * (beta as the last block left it), both halves from the one register: op_sel_hi[0] = 0.  (Nothing the
    # prefetch writes is read here, and fx is at least two instructions old on either path: no wait state.)
    for h in range(NP):
        g.emit(f"v_pk_mul_f32 {B[h]}, {g.txt(FXP)}, {g.txt(R[0][h])} op_sel_hi:[0,1]", [B[h]], [FX, R[0][h]], "pk")
    # masks: OR over the wave of the block's code bits = lane 0's | lane 63's (the wave holds at most two rows)
    g.emit(f"v_readfirstlane_b32 {S_A}, {g.txt(CODES)}", [], [CODES], "lane")
    g.emit(f"v_readlane_b32 {S_B}, {g.txt(CODES)}, 63", [], [CODES], "lane")
    g.emit(f"s_or_b32 {S_U}, {S_A}, {S_B}", kind="salu")
    g.emit(f"s_lshr_b32 {S_TMP}, {S_U}, 1", kind="salu")
    g.emit(f"s_or_b32 {S_NH}, {S_U}, {S_TMP}", kind="salu")
    g.emit(f"s_and_b32 {S_NH}, {S_NH}, 0x5555", kind="salu")
    g.emit(f"s_cmp_eq_u32 {S_NH}, 0", kind="salu")
    mixed = g.newlabel("mixed")
    nxt = g.newlabel("next")
    g.emit(f"s_cbranch_scc0 {mixed}", kind="branch")

    cold = []  # out-of-line bodies of the mixed path: (label, emitter function)

    # ---- suf(v.*w) of a site, kept from the beta pass for the forward pass ------------------------------------------------
    # The beta pass computes suf(v.*w_i) for the beta recursion, the forward pass needs the same vector again for gu: a site
    # whose vector survives in registers saves the forward pass its eleven instructions (four fmas, the lane total, the carry,
    # four adds).  Registers for that, per block kind (the plan at a block's entry and exit is the same for both):
    #   site 0       its vector is the last one the beta pass computes: it simply stays in the Z chain;
    #   SAVED sets   Tt (the state lives in the Z chain and in consumed w vectors during the forward pass, below);  the address /
    #                scale pairs of enter() with the Z chain's own total and carry (the beta pass borrows the Y chain's, idle
    #                there);  and, in an all-hom block only, the scalars of enter() and of the cold bodies (TAIL).
    # The state of the forward pass: a_0 = A (the checkpoint);  p of site 0 goes to the Z chain (site 0's vector has been used by
    # then, and the Z chain is computed again only from the first site without a saved vector on);  p of site i >= 1 goes to
    # R[i] = w of site i - 1, consumed one site earlier.
    #   PARKED       an all-hom block parks w of sites 5 and 6 (R[6], R[7]: written first by the beta pass, read last by the forward
    #                pass) in the thread's LDS slice, in the sixteen floats where the C++ body parks its two vectors, as soon as
    #                the beta pass has read them; their registers then keep the vectors of sites 4 and 5.  The forward pass
    #                asks for a parked w one site ahead, right after the kept vector in its registers has been used.
    SAVED_HOM = {1: Tt, 2: [ADDR, FXP, LTZ, CZ], 3: TAIL, 4: R[6], 5: R[7]}
    SAVED_MIXED = {1: Tt, 2: [ADDR, FXP, LTZ, CZ]}
    PARK_BYTE = (28 + 24) * 4  # the slice: emission table (Lane::ETAB_STRIDE = 28 floats), three mass rows, the parked vectors
    PARKED = {6: PARK_BYTE, 7: PARK_BYTE + 32}  # R[j] -> byte offset in the slice
    #   LDS_KEPT     an all-hom block also keeps the vector of site 6, for which no register is left: the beta pass computes it in the
    #                Z chain's own registers (two quads) and writes it to the eight floats of the slice behind the parked vectors
    #                (psmc_kernels.hip, sweep_run_kept: the C++ bodies never touch them); the forward pass asks it back into Tt as soon
    #                as site 1 has used the vector kept there, five sites before it is read, and the waits for the parked w vectors
    #                of sites 5 and 6 cover it (a wave's LDS accesses complete in order).  Site 7 is the one site whose vector is
    #                still computed twice: the slice has four floats left, a vector is eight.
    SLICE_FLOATS = 76  # sweep_lds_stride of these kernels: 19 units of 16 bytes, odd -- no bank conflict among the lanes of a ds_read_b128
    KEEP_BYTE = PARK_BYTE + 64
    LDS_KEPT = {6: (KEEP_BYTE, Tt, 1)}  # site -> (byte offset, the four pairs it comes back to, the site that frees them)
    assert KEEP_BYTE + 32 <= SLICE_FLOATS * 4 and Tt[0][1] % 4 == 0 and ZQ[0][1] % 4 == 0

    def park(j, store):
        for q in range(2):
            quad = ("q", R[j][2 * q][1])
            off = PARKED[j] + 16 * q
            assert off + 16 <= KEEP_BYTE
            if store:
                g.emit(f"ds_write_b128 {LDS}, {g.txt(quad)} offset:{off}", [], [LDS, quad], "lds")
            else:
                g.emit(f"ds_read_b128 {g.txt(quad)}, {LDS} offset:{off}", [quad], [LDS], "lds")

    def keep(i, store):
        off, back, _ = LDS_KEPT[i]
        for q in range(2):
            if store:  # (ZC[0..3] are the two quads of the Z chain, in this order)
                g.emit(f"ds_write_b128 {LDS}, {g.txt(ZQ[q])} offset:{off + 16 * q}", [], [LDS, ZQ[q]], "lds")
            else:
                quad = ("q", back[2 * q][1])
                g.emit(f"ds_read_b128 {g.txt(quad)}, {LDS} offset:{off + 16 * q}", [quad], [LDS], "lds")

    def beta_site(i, tests, ZC):
        """ZC: the four pairs of the site's Z chain (the chain's own registers, or a SAVED set)"""
        LTZ = LTY
        Wi = W(i)
        Bn = R[i]
        if tests:
            lab = g.newlabel(f"bh{i}")
            ret = g.newlabel(f"br{i}")
            # (no wait state behind the label: what reads w next is packed, not DPP, and is two instructions -- the test -- behind w's
            # last write on the fall-through and one -- the branch back -- behind the cold body's)
            g.emit(f"s_bitcmp1_b32 {S_NH}, {2 * i}", kind="salu")
            g.emit(f"s_cbranch_scc1 {lab}", kind="branch")
            g.label(ret)
            cold.append(("beta", i, lab, ret))
        # suffix of v.*w (Z chain) and prefix of b.*w (X chain), interleaved
        g.pk_fma(ZC[0], Pv[3], Wi[3], None)
        g.pk_fma(XC[0], Pb[0], Wi[0], None)
        g.pk_fma(ZC[1], Pv[2], Wi[2], ZC[0])
        g.pk_fma(XC[1], Pb[1], Wi[1], XC[0])
        g.pk_fma(ZC[2], Pv[1], Wi[1], ZC[1])
        g.pk_fma(XC[2], Pb[2], Wi[2], XC[1])
        # (tv goes to a register of the site's result, dead until the site's last instructions write it: the carry can then land
        # in ZC[3] itself, which is where svw3 = 0 + cv is read)
        TV = Bn[3]
        g.pk_fma(TV, Pv[0], Wi[0], ZC[2])      # tv
        g.pk_fma(XC[3], Pb[3], Wi[3], XC[2])   # tb
        g.lane_total(LTZ, TV)
        g.lane_total(LTX, XC[3])
        # nb_h = fma(d_h, w_h, pbw_h): pbw = (0, X0, X1, X2)  (independent work between the totals and the DPP reads)
        g.pk_fma(YC[0], Pd[0], Wi[0], None)
        g.pk_fma(YC[1], Pd[1], Wi[1], XC[0])
        g.pk_fma(YC[2], Pd[2], Wi[2], XC[1])
        g.pk_fma(YC[3], Pd[3], Wi[3], XC[2])
        g.carry(ZC[3], LTZ, TV, DN1, prefix=False)   # cv
        g.carry(CX, LTX, XC[3], UP1, prefix=True)    # cb
        # svw_h += cv: svw = (Z2, Z1, Z0, 0)
        CZ = g.seed(None, ZC[3])         # svw3 = 0 + cv   (the C++ source: splat(0) + cv)
        g.pk_add(ZC[0], ZC[0], CZ)       # svw2
        g.pk_add(ZC[1], ZC[1], CZ)       # svw1
        g.pk_add(ZC[2], ZC[2], CZ)       # svw0
        # nb += cb ; beta = fma(u, svw, nb)
        for h in range(NP):
            g.pk_add(YC[h], YC[h], CX)
        svw = [ZC[2], ZC[1], ZC[0], ZC[3]]
        for h in range(NP):
            g.pk_fma(Bn[h], Pu[h], svw[h], YC[h])

    def fwd_site(i, tests, a, t, kept, refill=None, wait=False):
        """a: registers of the state entering the site; t: where p = A' a goes (the next site's a); kept: the four pairs that hold
        the site's Z chain from the beta pass (None: it is computed here, in the Z chain's own registers); refill: the R[j] to
        read back from LDS once `kept` has been used; wait: this site's w was asked for by the site before"""
        Wi = W(i)
        last = i == T - 1
        if wait and kept is None:  # (the Z chain reads w at once)
            g.emit("s_waitcnt lgkmcnt(0)", kind="wait")
        if kept is not None:
            # the chains of u.*a and a alone; the site's gu and gd rows need no scan of this pass and fill the chains' gaps
            svw = [kept[2], kept[1], kept[0], kept[3]]
            g.pk_fma(XC[0], Pu[0], a[0], None)
            Y0 = g.seed(YC[0], a[3])               # 0 + a3
            g.pk_fma(GU[0], a[0], svw[0], GU[0])
            g.pk_fma(XC[1], Pu[1], a[1], XC[0])
            g.pk_add(YC[1], Y0, a[2])
            g.pk_fma(GU[1], a[1], svw[1], GU[1])
            g.pk_fma(XC[2], Pu[2], a[2], XC[1])
            g.pk_add(YC[2], YC[1], a[1])
            g.pk_fma(GU[2], a[2], svw[2], GU[2])
            g.pk_fma(XC[3], Pu[3], a[3], XC[2])    # tu
            g.pk_add(YC[3], YC[2], a[0])           # ta
            g.pk_fma(GU[3], a[3], svw[3], GU[3])
            g.lane_total(LTX, XC[3])
            g.lane_total(LTY, YC[3])
            if wait:  # (nothing above reads w: the wait stands behind fourteen instructions of this site and before the next request)
                g.emit("s_waitcnt lgkmcnt(0)", kind="wait")
            if refill is not None:  # the kept vector has been used: its registers take back the parked w the next site reads
                park(refill, store=False)
        else:
            g.pk_fma(XC[0], Pu[0], a[0], None)
            Y0 = g.seed(YC[0], a[3])               # 0 + a3
            g.pk_fma(ZC[0], Pv[3], Wi[3], None)
            g.pk_fma(XC[1], Pu[1], a[1], XC[0])
            g.pk_add(YC[1], Y0, a[2])
            g.pk_fma(ZC[1], Pv[2], Wi[2], ZC[0])
            g.pk_fma(XC[2], Pu[2], a[2], XC[1])
            g.pk_add(YC[2], YC[1], a[1])
            g.pk_fma(ZC[2], Pv[1], Wi[1], ZC[1])
            g.pk_fma(XC[3], Pu[3], a[3], XC[2])    # tu
            g.pk_add(YC[3], YC[2], a[0])           # ta
            g.pk_fma(ZC[3], Pv[0], Wi[0], ZC[2])   # tv
            g.lane_total(LTX, XC[3])
            g.lane_total(LTY, YC[3])
            g.lane_total(LTZ, ZC[3])
        # gd += w .* a (needs nothing of the scans: fills the gap before the DPP reads)
        for h in range(NP):
            g.pk_fma(GD[h], Wi[h], a[h], GD[h])
        g.carry(CX, LTX, XC[3], UP1, prefix=True)     # cu
        g.carry(CY, LTY, YC[3], DN1, prefix=False)    # ca
        if kept is None:
            g.carry(CZ, LTZ, ZC[3], DN1, prefix=False)    # cv
        # pre = (0, X0, X1, X2) + cu ; suf = (Y2, Y1, Y0, 0) + ca ; svw = (Z2, Z1, Z0, 0) + cv
        # (the three 0 + carry entries are the carries themselves, read where they stand: nothing writes cu, ca, cv before the next
        # site's carries, behind every read of this site;  Y0 + ca reads a3, which the site's last instructions still need, and
        # writes the chain's own register)
        X3 = g.seed(XC[3], CX)
        Y3 = g.seed(YC[3], CY)
        if kept is None:
            Z3 = g.seed(ZC[3], CZ)
        for k in range(3):
            g.pk_add(XC[k], XC[k], CX)
            g.pk_add(YC[k], Y0 if k == 0 else YC[k], CY)
            if kept is None:
                g.pk_add(ZC[k], ZC[k], CZ)
        pre = [X3, XC[0], XC[1], XC[2]]
        suf = [YC[2], YC[1], YC[0], Y3]
        for h in range(NP):
            g.pk_fma(GB[h], Wi[h], suf[h], GB[h])
        for h in range(NP):
            g.pk_fma(GV[h], Wi[h], pre[h], GV[h])
        if kept is None:
            svw = [ZC[2], ZC[1], ZC[0], Z3]
            for h in range(NP):
                g.pk_fma(GU[h], a[h], svw[h], GU[h])
        if last and not tests:
            return
        for h in range(NP):
            g.pk_mul(t[h], Pd[h], a[h])
        for h in range(NP):
            g.pk_fma(t[h], Pv[h], pre[h], t[h])
        for h in range(NP):
            g.pk_fma(t[h], Pb[h], suf[h], t[h])
        if tests:
            lab = g.newlabel(f"fh{i}")
            ret = g.newlabel(f"fr{i}")
            g.emit(f"s_bitcmp1_b32 {S_NH}, {2 * i}", kind="salu")
            g.emit(f"s_cbranch_scc1 {lab}", kind="branch")
            g.label(ret)
            cold.append(("fwd", i, lab, ret, t))

    def block(tests):
        saved = SAVED_MIXED if tests else SAVED_HOM
        parks = not tests
        for i in range(T - 1, -1, -1):
            beta_site(i, tests, saved.get(i, ZC))
            if parks and i + 1 in PARKED:  # w of site i (R[i + 1]) has just been read for the last time in this pass
                park(i + 1, store=True)
            if parks and i in LDS_KEPT:    # the site's vector stands in the Z chain, which the next sites of this pass leave alone
                assert all(j in saved for j in range(1, i))
                keep(i, store=True)
        a = A
        for i in range(T):
            t = ZC if i == 0 else R[i]
            kept = ZC if i == 0 else saved.get(i)
            if parks and i in LDS_KEPT:
                kept = LDS_KEPT[i][1]
            # (site i's kept vector sits in R[i + 2], the registers of w of site i + 1: asked back as soon as the vector is used)
            fwd_site(i, tests, a, t, kept, refill=i + 2 if parks and i + 2 in PARKED else None, wait=parks and i + 1 in PARKED)
            if parks:
                for j, (_, back, free) in LDS_KEPT.items():
                    if free == i:
                        # (a site between the two waits for its parked w: that wait is the one that covers this read)
                        assert back is saved[i] and any(n + 1 in PARKED for n in range(i + 1, j))
                        keep(j, store=False)
            a = t
        # (the block's result, beta at its left edge, stays in R[0]: see the run's prologue)

    # ---- all-hom block ---------------------------------------------------------------------------------------------------
    block(False)
    g.emit(f"s_branch {nxt}", kind="branch")
    # ---- mixed block -----------------------------------------------------------------------------------------------------
    g.label(mixed)
    g.emit(f"s_and_b32 {S_NM}, {S_TMP}, 0x5555", kind="salu")   # bit 2i: site i is missing in some lane (only this body asks)
    block(True)
    g.label(nxt)
    g.emit(f"s_sub_i32 {BLK}, {BLK}, 1", kind="salu")
    g.emit(f"s_cmp_ge_i32 {BLK}, {STOP}", kind="salu")
    g.emit(f"s_cbranch_scc1 {top}", kind="branch")
    done = g.newlabel("done")
    g.emit(f"s_branch {done}", kind="branch")

    # ---- cold bodies of the mixed block ----------------------------------------------------------------------------------
    for c in cold:
        if c[0] == "beta":
            _, i, lab, ret = c
            Wi = W(i)
            g.label(lab)
            g.emit("s_nop 1", kind="salu")
            g.emit(f"v_bfe_u32 {g.txt(CC)}, {g.txt(CODES)}, {2 * i}, 2", [CC], [CODES])
            g.emit("s_nop 0", kind="salu")
            g.emit(f"v_cmp_eq_u32_e32 vcc, 1, {g.txt(CC)}", [], [CC])
            g.emit(f"s_and_saveexec_b64 {S_SAVE}, vcc", kind="salu")
            for h in range(NP):
                g.pk_mul(Wi[h], Wi[h], RH[h])
            g.emit(f"s_mov_b64 exec, {S_SAVE}", kind="salu")
            g.emit(f"s_bitcmp1_b32 {S_NM}, {2 * i}", kind="salu")
            g.emit(f"s_cbranch_scc0 {ret}", kind="branch")
            # a missing site: w .*= row (1 / emis0 where this lane's site is missing, row 0 = ones elsewhere)
            g.emit(f"v_cmp_eq_u32_e32 vcc, 2, {g.txt(CC)}", [], [CC])
            g.emit(f"v_cndmask_b32_e64 {g.txt(LADDR)}, 0, 64, vcc", [LADDR], [])
            g.emit(f"v_add_u32_e32 {g.txt(LADDR)}, {LDS}, {g.txt(LADDR)}", [LADDR], [LADDR, LDS])
            g.emit("s_nop 0", kind="salu")
            g.emit(f"ds_read_b128 {g.txt(ER0)}, {g.txt(LADDR)}", [ER0], [LADDR], "lds")
            g.emit(f"ds_read_b128 {g.txt(ER1)}, {g.txt(LADDR)} offset:16", [ER1], [LADDR], "lds")
            g.emit("s_waitcnt lgkmcnt(0)", kind="wait")
            for h in range(NP):
                q = ER0 if h < 2 else ER1
                e = ("p", q[1] + 2 * (h % 2))
                g.pk_mul(Wi[h], Wi[h], e)
            g.emit(f"s_branch {ret}", kind="branch")
        else:
            _, i, lab, ret, t = c
            Wi = W(i)
            g.label(lab)
            g.emit("s_nop 1", kind="salu")
            g.emit(f"v_bfe_u32 {g.txt(CC)}, {g.txt(CODES)}, {2 * i}, 2", [CC], [CODES])
            g.emit("s_nop 0", kind="salu")
            g.emit(f"v_cmp_eq_u32_e32 vcc, 1, {g.txt(CC)}", [], [CC])
            g.emit(f"s_and_saveexec_b64 {S_SAVE}, vcc", kind="salu")
            for h in range(NP):
                g.pk_fma(G1[h], t[h], Wi[h], G1[h])
            for h in range(NP):
                g.pk_mul(t[h], t[h], RH[h])
            g.emit(f"s_mov_b64 exec, {S_SAVE}", kind="salu")
            g.emit(f"s_bitcmp1_b32 {S_NM}, {2 * i}", kind="salu")
            g.emit(f"s_cbranch_scc0 {ret}", kind="branch")
            # a missing site: mass p .* w into the LDS row of the lane's code (2, or 0 where this lane is not missing: nobody
            # reads row 0), then p .*= the lane's emission row
            g.emit(f"v_cmp_eq_u32_e32 vcc, 2, {g.txt(CC)}", [], [CC])
            g.emit(f"v_cndmask_b32_e64 {g.txt(LADDR)}, 0, 64, vcc", [LADDR], [])
            g.emit(f"v_add_u32_e32 {g.txt(LADDR)}, {LDS}, {g.txt(LADDR)}", [LADDR], [LADDR, LDS])
            g.emit("s_nop 0", kind="salu")
            g.emit(f"ds_read_b128 {g.txt(GR0)}, {g.txt(LADDR)} offset:112", [GR0], [LADDR], "lds")
            g.emit(f"ds_read_b128 {g.txt(GR1)}, {g.txt(LADDR)} offset:128", [GR1], [LADDR], "lds")
            g.emit(f"ds_read_b128 {g.txt(ER0)}, {g.txt(LADDR)}", [ER0], [LADDR], "lds")
            g.emit(f"ds_read_b128 {g.txt(ER1)}, {g.txt(LADDR)} offset:16", [ER1], [LADDR], "lds")
            g.emit("s_waitcnt lgkmcnt(0)", kind="wait")
            for h in range(NP):
                q = GR0 if h < 2 else GR1
                gr = ("p", q[1] + 2 * (h % 2))
                g.pk_fma(gr, t[h], Wi[h], gr)
            for h in range(NP):
                q = ER0 if h < 2 else ER1
                e = ("p", q[1] + 2 * (h % 2))
                g.pk_mul(t[h], t[h], e)
            g.emit("s_nop 0", kind="salu")
            g.emit(f"ds_write_b128 {g.txt(LADDR)}, {g.txt(GR0)} offset:112", [], [LADDR, GR0], "lds")
            g.emit(f"ds_write_b128 {g.txt(LADDR)}, {g.txt(GR1)} offset:128", [], [LADDR, GR1], "lds")
            g.emit(f"s_branch {ret}", kind="branch")

    g.label(done)
    g.emit("s_waitcnt vmcnt(0) lgkmcnt(0)", kind="wait")
    for h in range(NP):
        g.mov64(B[h], R[0][h])
    for i in range(4):
        g.emit(f"v_mov_b32_e32 {AN[i]}, {g.txt(quad_lane(PQ0, i))}", [AN[i]], [quad_lane(PQ0, i)])
        g.emit(f"v_mov_b32_e32 {AN[4 + i]}, {g.txt(quad_lane(PQ1, i))}", [AN[4 + i]], [quad_lane(PQ1, i)])
    lines, nops = g.finish()
    return lines, nops, g.next_free, {"slice_floats": SLICE_FLOATS, "seeds_aliased": g.seeds_aliased}


def path_counts(lines):
    """Instruction mix of one trip through the block loop, per kind of block: {"all-hom" | "mixed": {class: count}}.  The mixed
    trip is the one whose sixteen tests all fall through (the cold bodies are out of line, behind the loop); both trips take the
    checkpoint prefetch and skip the step into the next observation word (every second block takes its nine instructions)."""
    def stem(ln):
        return ln.split("_")[1] if ln.startswith(".Lphk_") else None

    pos = {}
    for n, ln in enumerate(lines):
        if ln.endswith(":"):
            pos.setdefault(stem(ln), n)
    skip_from = next(n for n, ln in enumerate(lines) if ln.startswith("s_cbranch_scc0") and stem(ln.split()[1]) == "sameword")
    enter = [ln for n, ln in enumerate(lines[pos["top"]:pos["mixed"]], pos["top"]) if not (skip_from < n < pos["sameword"])]
    split = next(n for n, ln in enumerate(enter) if ln.startswith("s_cbranch_scc0") and stem(ln.split()[1]) == "mixed")
    hom = enter[split + 1:]
    enter = enter[:split + 1]
    tail = lines[pos["next"]:next(n for n in range(pos["next"], len(lines)) if lines[n].startswith("s_cbranch_scc1")) + 1]
    mixed = lines[pos["mixed"]:pos["next"]]
    res = {}
    for name, body in (("all-hom", enter + hom + tail), ("mixed", enter + mixed + tail)):
        ins = [ln.split()[0] for ln in body if not ln.endswith(":")]
        res[name] = {
            "total": len(ins),
            "vector": sum(m.startswith("v_") for m in ins),
            "packed": sum(m.startswith("v_pk_") for m in ins),
            "scalar": sum(m.startswith("s_") and not m.startswith(("s_cbranch", "s_branch", "s_nop", "s_waitcnt")) for m in ins),
            "branch": sum(m.startswith(("s_cbranch", "s_branch")) for m in ins),
            "s_nop": sum(m == "s_nop" for m in ins),
            "waitcnt": sum(m == "s_waitcnt" for m in ins),
            "LDS": sum(m.startswith("ds_") for m in ins),
            "global": sum(m.startswith("global_") for m in ins),
        }
    return res


def main():
    lines, nops, top, info = build()
    for name, c in path_counts(lines).items():
        print(f"{name} block: " + ", ".join(f"{k} {v}" for k, v in c.items()))
    print(f"LDS slice: {info['slice_floats']} floats per thread; scan seeds read in place (no x + 0): {info['seeds_aliased']} in the two bodies")
    if len(sys.argv) > 1 and sys.argv[1] == "--report":
        return
    out = sys.argv[1] if len(sys.argv) > 1 else "phlash_amd/csrc/sweep_run_k16r2.inc"
    ops_io = []
    for nm, var in (("b", "beta"), ("gb", "gb"), ("gd", "gd"), ("gu", "gu"), ("gv", "gv"), ("g1", "g1")):
        ops_io += [f'[{nm}{h}] "+v"({var}[{h}])' for h in range(NP)]
    ops_io += [f'[an{i}] "+v"(anext[{i}])' for i in range(8)]
    ops_io += ['[wcur] "+v"(wcur)', '[wprev] "+v"(wprev)', '[enext] "+v"(e_next)', '[ckq] "+v"(asm_ckq)', '[ebq] "+v"(asm_ebq)',
               '[blk] "+s"(asm_blk)', '[widx] "+s"(asm_widx)']
    ops_in = []
    for nm, var in (("pb", "lane.b"), ("pd", "lane.d"), ("pu", "lane.u"), ("pv", "lane.v"), ("rh", "rhet")):
        ops_in += [f'[{nm}{h}] "v"({var}[{h}])' for h in range(NP)]
    ops_in += ['[up1] "v"(lane.g.upm1)', '[dn1] "v"(lane.g.dnm1)', '[words] "v"(asm_words)', '[lds] "v"(asm_lds)', '[stop] "s"(asm_stop)',
               '[blklo] "s"(asm_blklo)', '[ckstep] "s"(asm_ckstep)', '[ebstep] "s"(asm_ebstep)', '[ckpiece] "s"(asm_ckpiece)']
    clob = [f'"v{i}"' for i in range(TBASE, 256)] + [f'"s{i}"' for i in range(86, 100)] + ['"vcc"', '"scc"', '"memory"']
    with open(out, "w") as f:
        f.write("// GENERATED by scripts/gen_sweep_asm.py -- do not edit.  The run of hot blocks of bwd_kernel<float, 16, 2, 8, 4, *> as one asm\n"
                f"// statement ({len(lines)} lines, {nops} s_nop inserted by the generator's hazard pass, temporaries v{TBASE}..v{top - 1}).\n")
        f.write("asm volatile(\n")
        for ln in lines:
            f.write(f'    "{ln}\\n\\t"\n')
        f.write("    : " + ", ".join(ops_io) + "\n    : " + ", ".join(ops_in) + "\n    : " + ", ".join(clob) + ");\n")
    print(f"wrote {out}: {len(lines)} lines, {nops} s_nop, temporaries up to v{top - 1}")


if __name__ == "__main__":
    main()
