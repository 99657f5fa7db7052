// The body of fwd_kernel / fwd_kernel_mr (psmc_kernels.hip), included once per kernel with PHK_KERNEL_MR = false / true: two real
// definitions, so that the kernel launched for rows without runs of missing sites is compiled from exactly the text it always was
// (a shared forceinline function changed the code of both, and brought AGPR copies + scratch into two float64 kernels).
    using L = Lane<real, K, R>;
    using V = typename L::V;
    constexpr int SPL = L::SPL, NP = L::NP;
    static_assert(T <= 16 && 16 % T == 0, "a block's codes must sit in one dword");
    static_assert(T % NRM == 0, "the rescale schedule must restart with every block");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
#if PHK_FWD_PRIO
    if constexpr (CKPT && !has_dense<real, K, R>()) __builtin_amdgcn_s_setprio(PHK_FWD_PRIO);
#endif
    const int64_t nseq = A.B * A.S;
    const int rank = threadIdx.x & (R - 1);
    // A wave none of whose lane groups has a sequence leaves (wave-uniform; these kernels have no barrier).  It must
    // not run: lane groups without a sequence repeat another sequence's work and, in the lean piece loops, its
    // stores -- harmless inside a wave that also holds the real group (same wave votes, hence the same dense /
    // structured steps, the same rescales, the same bits to the same addresses), but a wave made of repeats only
    // votes among copies of ONE sequence, takes dense steps and rescales where the real group's wave does not, and its
    // checkpoints and block exponents -- scaled by other powers of two -- would race with the real ones (seen in the
    // fuzz soak once the dense steps stopped rescaling after every step: the last sequence of a launch came back with
    // checkpoints of one scaling and exponents of the other).
    const SeqMap sm = map_group<real, K, R>(A);
#ifndef PHK_KEEP_IDLE_WAVES  // (diagnostic builds define it to show that the regression test catches the race)
    if (sm.idle_wave) return;
#endif
    const bool active = sm.active;
    const int64_t bb = sm.bb, ss = sm.ss, seq = sm.seq;

    L lane;
    V a[NP];
    lane.load((const real*)A.params + bb * A.pstride_b + ss * A.pstride_s, rank,
              (real*)smem_raw + (size_t)threadIdx.x * L::ETAB_STRIDE, a);
    const real* pfb = prefold_block<real>(A, bb, ss);
    const bool fold_seq = lane.try_fold(pfb != nullptr ? pfb + rank * L::SPL : nullptr);  // (float32: the folded model, see Lane::try_fold)
    constexpr bool DENSE = has_dense<real, K, R>() && NRM == 4;  // hom-run operators (see dense16)
    // Several states per lane, NRM = 4: the full blocks (straight_block, fold_block) rescale on demand -- the rescale
    // sites of the schedule only test the sum the site's own scan has produced, and a sequence is rescaled once it
    // has lost 2^-PHK_RESCALE_TRIGGER_EXP (Lane::rescale_on_demand).  Most blocks record an exponent of 0; E, eblk, eseg
    // and eb_min stay "the exponent actually removed".  The partial last block and the warm-up block keep the fixed
    // schedule, NRM = 1 and 2 keep theirs bit for bit, and the one-state-per-lane kernels rescale by debt (dense_block).
    constexpr bool ONDEMAND = NRM == 4 && SPL > 1 && PHK_RESCALE_TRIGGER_EXP > 0;
    if constexpr (DENSE)
        lane.template load_dense<T == 16>(A.ops_f + (A.pstride_s != 0 ? bb * A.S + ss : bb) * DENSE_OPS_FLOATS, rank, fold_seq,
                                          PHK_KERNEL_MR ? (float*)smem_raw + (size_t)blockDim.x * L::ETAB_STRIDE + (size_t)threadIdx.x * DENSE_Q8_STRIDE : nullptr);
    const uint32_t* words = A.packed + checked_row(A, ss) * A.Lw;
    // Do the four sequences of this wave read ONE observation row (true for every wave of a range of whole particles:
    // map_group), and are their hom emissions far enough from zero for the het / missing ratios to exist?  Then the codes are scalars and every run of sites is one
    // dense step (uni_block below).  Other waves keep the wave-vote path.
    bool uni = false;
    if constexpr (DENSE && PHK_DENSE_UNI != 0) {
        const int ss0 = __builtin_amdgcn_readfirstlane((int)ss);
        uni = __all((int)ss == ss0 && (fold_seq || lane.etab[0] > RATIO_MIN_EMIS0)) != 0;
    }
    // The other float32 layouts: sequences are stored chunk-major (SeqMap), so a wave holds the particles of ONE chunk,
    // or of two where it crosses a chunk boundary.  Such a wave (uni2) folds its hom emission into the factors
    // (Lane::fold_emissions) and takes its codes as scalars: a block of T sites that is hom in both rows -- 85 % of the
    // blocks at 1 % hets -- runs without a single emission row (no LDS gather, no multiply: a timing-only build of the
    // one-lane forward kernel without them ran cfg2's forward phase in 8.1 instead of 10.8 ms); any other block takes
    // the straight-line path with per-lane codes as ever, its rows now the ratios emis1 / emis0, 1 / emis0 and 1.
    constexpr bool FOLD = !DENSE && (sizeof(real) == 4 || PHK_FOLD_F64 != 0) && PHK_FWD_FOLD != 0;
    constexpr bool FREG = FOLD && PHK_FWD_HET_REGS != 0;
    V rhet[NP], rmis[NP];  // FREG: a folded lane's ratio rows emis1 / emis0 and 1 / emis0 (see fold_block)
    if constexpr (FREG) {
#pragma unroll
        for (int h = 0; h < NP; ++h) {
            rhet[h] = *(const V*)(lane.etab + L::EROW + 2 * h);
            rmis[h] = *(const V*)(lane.etab + 2 * L::EROW + 2 * h);
        }
    }
    bool uni2 = false, rowB = false;
    if constexpr (FOLD) {
        const int sA = __builtin_amdgcn_readfirstlane((int)ss), sB = __builtin_amdgcn_readlane((int)ss, 63);
        // (a sequence folds whenever its own ratios exist, whatever its wave does: a site's row is then exactly 1 where
        // the wave-uniform path would have skipped the multiply, so both paths return the same bits)
        uni2 = __all(((int)ss == sA || (int)ss == sB) && fold_seq) != 0;
        rowB = (int)ss != sA;
    }

    int E = 0;
    // smallest distance to its threshold of any exponent a rescale of this sequence removed: RISK_EXP_* for the
    // rescales after NRM sites, RISK_EXP_DEFERRED_F32 for the deferred rescales of the dense steps.  ONE variable on
    // purpose: with two, the compiler sinks the updates into one block behind a select of their ADDRESSES, both stay
    // in scratch, and every scratch_load's s_waitcnt vmcnt(0) also waits for the observation piece requested ahead
    // (round 4: 35-42 % of the one-state-per-lane kernels' wave cycles went there)
    constexpr int RISK_EXP = sizeof(real) == 4 ? RISK_EXP_F32 : RISK_EXP_F64;
    int ex_slack = 1 << 20;
    int hom_run = 0;  // dense kernels: rescale debt -- hom sites stepped over since the last rescale (uniform path: + 16 per het / missing site)
    int eb_min = 0;   // smallest exponent total of any checkpoint block
    double llW = 0.0;
    // Block loop bookkeeping is kept in 32-bit wave-uniform integers and stepped pointers: in the
    // latency-bound layout a block is only ~300 cycles of arithmetic, and 64-bit index products or
    // an integer division per block (the segment test used to be blk % seg_blocks) cost as much.
    const int nblk = (int)((A.Ltot + T - 1) / T);
    const int nfull = (int)(A.Ltot / T);                      // blocks [0, nfull) hold T sites
    const int tail = (int)(A.Ltot - (int64_t)nfull * T);      // sites of the last, partial block
    const int blkW = A.W > 0 ? (int)((A.W - 1) / T) : -1;     // block holding the warm-up boundary
    const int iW = A.W > 0 ? (int)((A.W - 1) - (int64_t)blkW * T) : -1;  // ... after its site iW
    const int64_t ck_step = nseq * K;
    real* ckp = (real*)A.ckpt + L::ck_lane(nseq, seq, rank);   // this lane's first state in the current block's checkpoint
    int16_t* ebp = A.eblk + seq;
    int32_t* esp = A.eseg + seq;
    int seg_left = 0;  // blocks until the next segment starts
    // Observation words come in 16-byte pieces (4 words = 64 sites; rows are padded to whole
    // pieces), requested one piece ahead, and the block loop is nested inside the piece loop.  The
    // wait for a piece also waits for every store issued before it completes (vmcnt counts stores,
    // and the checkpoint stores sit in branches the compiler cannot count through): with the
    // prefetched word carried around a flat block loop that was a full store round trip per block.
    constexpr int BPC = 64 / T;  // blocks per piece
    const uint4* pieces = (const uint4*)words;
    const int npieces = (int)(A.Lw >> 2);
    uint4 pnext = pieces[0];
    // land the first piece before the loop (an empty asm that reads it): otherwise "the register of
    // the current piece may still be in flight" is a state the compiler carries around the block loop,
    // and it waits (vmcnt) before every block's word select -- which also drains that block's
    // checkpoint stores.  float32 kernels only: the float64 K = 64 forward kernel (pieces and
    // parameters loaded straight into AGPRs, scratch in use) returned wrong log-likelihoods with it,
    // in this form and with an explicit s_waitcnt alike, and passes without.
    if constexpr (sizeof(real) == 4 || PHK_EXP_LAND_F64) asm volatile("" ::"v"(pnext.x), "v"(pnext.y), "v"(pnext.z), "v"(pnext.w));
    // With checkpoint stores in flight, every wait for a requested piece is a wait for ALL stores issued
    // before it (one store round trip, ~5,000 cycles under the 2 TB/s this kernel writes: 19 % of a lone
    // wave's cycles at one wait per 64 sites).  The checkpointing variants that have registers to spare
    // therefore request FOUR pieces (256 sites) at a time and pay that round trip a quarter as often.
    constexpr int PPB = ((PHK_FWD_BIG_PIECES == 1 && CKPT && !has_dense<real, K, R>() && SPL * (int)sizeof(real) >= 32) ||
                         (PHK_FWD_BIG_PIECES == 2 && CKPT && has_dense<real, K, R>())) ? 4 : 1;
    uint4 nx1 = pnext, nx2 = pnext, nx3 = pnext;
    if constexpr (PPB == 4) {
        nx1 = pieces[1 < npieces ? 1 : npieces - 1];
        nx2 = pieces[2 < npieces ? 2 : npieces - 1];
        nx3 = pieces[3 < npieces ? 3 : npieces - 1];
        if constexpr (sizeof(real) == 4 || PHK_EXP_LAND_F64)
            asm volatile("" ::"v"(nx1.x), "v"(nx1.y), "v"(nx1.z), "v"(nx1.w), "v"(nx2.x), "v"(nx2.y), "v"(nx2.z), "v"(nx2.w),
                         "v"(nx3.x), "v"(nx3.y), "v"(nx3.z), "v"(nx3.w));
    }
    // One full block of the one-state-per-lane layout (DENSE): sixteen / eight / four / two hom sites for all
    // four sequences of the wave (wave vote) are ONE dense M_h^n step; one rescale per dense step, or per
    // group of four sites (the NRM = 4 schedule) where structured steps are needed.  All-hom blocks of 8 sites
    // are 61 % of the blocks at 5 % hets + 1 % missing, of 16 sites 37 %.  The block's exponent total goes
    // into eblk as ever; the sweep re-runs blocks in its own scaling and corrects beta by 2^(e_run - e_fwd).
    auto dense_block = [&](const uint32_t codes) {
        if constexpr (DENSE) {
            // A rescale costs as much as the dense step itself (sum butterfly, exponent, multiply: ~90 of ~240 dependent
            // cycles), and a hom site takes little mass away: along a run of dense steps the state is rescaled once per
            // PHK_DENSE_RESCALE_SITES sites.  Blocks in between record an exponent of 0; power-of-two scales round
            // nothing, so the checkpoints and the log-likelihood are the same bits times a power of two.
            if (T == 16 && PHK_DENSE16 && __all(codes == 0u)) {
                a[0][0] = dense16(a[0][0], lane.D16);
                hom_run += 16;
                if (hom_run >= PHK_DENSE_RESCALE_SITES) {
                    hom_run = 0;
                    const int ex = lane.rescale(a);
                    E += ex;
                    ex_slack = min(ex_slack, ex - RISK_EXP_DEFERRED_F32);
                }
                return;
            }
#pragma unroll
            for (int h8 = 0; h8 < T / 8; ++h8) {
                if (PHK_DENSE8 && __all(((codes >> (16 * h8)) & 0xffffu) == 0u)) {
                    a[0][0] = dense16(a[0][0], lane.P[7]);
                    hom_run += 8;
                    if (hom_run >= PHK_DENSE_RESCALE_SITES) {
                        hom_run = 0;
                        const int ex = lane.rescale(a);
                        E += ex;
                        ex_slack = min(ex_slack, ex - RISK_EXP_DEFERRED_F32);
                    }
                    continue;
                }
                hom_run = 0;  // (the groups of four below end in a rescale each)
#pragma unroll
                for (int g = 2 * h8; g < 2 * h8 + 2; ++g) {
                    const uint32_t c4 = (codes >> (8 * g)) & 0xffu;
                    if (__all(c4 == 0u)) {
                        a[0][0] = dense16(a[0][0], lane.P[3]);
                    } else {
#pragma unroll
                        for (int hh = 0; hh < 2; ++hh) {
                            const uint32_t c2 = (c4 >> (4 * hh)) & 0xfu;
                            if (__all(c2 == 0u)) {
                                a[0][0] = dense16(a[0][0], lane.P[1]);
                            } else {
                                real sc;
                                V e[NP];
                                lane.emis(c2 & 3, e);
                                lane.fwd_site(a, e, sc, false);
                                lane.emis(c2 >> 2, e);
                                lane.fwd_site(a, e, sc, false);
                            }
                        }
                    }
                    const int ex = lane.rescale(a);
                    E += ex;
                    ex_slack = min(ex_slack, ex - RISK_EXP);
                }
            }
        }
    };
    // One full block of a wave whose sequences share their observation row (uni): `rem` holds the block's codes as a
    // SCALAR.  A run "hom^(n-1), then a het or missing site" is one dense M_h^n step plus one multiply by emis1 / emis0
    // or 1 / emis0 (Lane::half_step: straight-line code for the all-hom half and for a half with one such site).
    // Rescales: when the debt (1 per hom site, 16 per het / missing site) reaches PHK_DENSE_RESCALE_SITES, i.e. after
    // at most 64 hom or 4 other sites as before.  Returns the exponent taken out of the block.
    auto uni_block = [&](const uint32_t rem) -> int {
        int dE = 0;
        if constexpr (DENSE) {
            float x = a[0][0];
            // (a rescale inside a block that holds het / missing sites comes after at most four of them, like a group of four
            // of the wave-vote path, and is held to the same threshold: 2^-80 out of four hets of emis1 / emis0 = 1e-6 passed
            // the deferred one, and the sweep behind it returned NaN with the flag clear -- tests/test_model_fuzz.py, REGRESSIONS)
            const int risk_exp = rem != 0u ? RISK_EXP_F32 : RISK_EXP_DEFERRED_F32;
            auto resc = [&](float& y) -> int {
                const int ex = lane.rescale1(y);
                dE += ex;
                ex_slack = min(ex_slack, ex - risk_exp);
                return 0;
            };
            if (T == 16 && __builtin_expect(rem == 0u, 1)) {
                x = dense16(x, lane.D16);
                hom_run += 16;
            } else {
                hom_run = lane.template half_step<true, PHK_KERNEL_MR>(x, rem & 0xffffu, hom_run, resc);
                if constexpr (T == 16) {
                    if (__builtin_expect(hom_run >= PHK_DENSE_RESCALE_SITES, 0)) hom_run = resc(x);
                    hom_run = lane.template half_step<true, PHK_KERNEL_MR>(x, rem >> 16, hom_run, resc);
                }
            }
            if (__builtin_expect(hom_run >= PHK_DENSE_RESCALE_SITES, 0)) hom_run = resc(x);
            a[0][0] = x;
        }
        return dE;
    };
    // one full block of the other layouts: a straight-line basic block of T sites (no per-site branches), the
    // emission row of the next site in flight while the current one computes
    auto straight_block = [&](const uint32_t codes) {
        V ec[NP];
        lane.emis(codes & 3, ec);
#pragma unroll
        for (int i = 0; i < T; ++i) {
            V en[NP];
            if (i + 1 < T) lane.emis((codes >> (2 * (i + 1))) & 3, en);
            real sc;
            if constexpr (ONDEMAND) {
                if (rescale_after<NRM>(i)) {
                    real sum_before;
                    lane.fwd_site_sum(a, ec, sum_before);
                    lane.template rescale_on_demand<RISK_EXP>(a, sum_before, E, ex_slack);
                } else {
                    lane.fwd_site(a, ec, sc, false);
                }
            } else {
                const int ex = lane.fwd_site(a, ec, sc, rescale_after<NRM>(i));
                E += ex;
                if (NRM > 1 && rescale_after<NRM>(i)) ex_slack = min(ex_slack, ex - RISK_EXP);
            }
            if (i + 1 < T) {
#pragma unroll
                for (int h = 0; h < NP; ++h) ec[h] = en[h];
            }
#if PHK_FWD_SITE_BARRIER
            __builtin_amdgcn_sched_barrier(0);
#endif
        }
    };
    // Lean piece loop of the DENSE kernels.  A block of this layout is ~500 cycles of arithmetic, and the
    // general block loop below spent as many again on its per-block tests (full block? warm-up boundary?
    // segment start? which word of the piece?), on 64-bit per-lane store addresses and on exec-mask branches
    // around the stores (timing-only builds at 500 x 5 x 100,000: 1.31 of 2.64 ms).  A piece of 64 sites that
    // holds only full blocks and no warm-up boundary takes this path instead: tests once per piece, the
    // piece's words rotated through one register, wave-uniform store bases with 32-bit lane offsets, and
    // stores by every lane (lanes past the last sequence repeat its work bit for bit: same value, same address).
    constexpr bool LEAN = PPB == 1 && (DENSE ? PHK_DENSE_LEAN != 0 : (PHK_FWD_LEAN != 0 && PHK_EMIS_AHEAD < 2));
    // (lane offsets of the lean stores are 32-bit BYTE offsets beside a wave-uniform base: the store then takes the
    // base from SGPRs -- global_store ... v_off, v_data, s[base] -- and costs no address arithmetic per block)
    const bool lean_ok = LEAN && (A.seg_blocks % BPC) == 0 && nseq * K * (int64_t)sizeof(real) < (int64_t(1) << 31);
    const unsigned ck_off_e = (unsigned)L::ck_lane(nseq, seq, rank), sq_off_e = (unsigned)seq;
    const unsigned ck_piece_e = (unsigned)(nseq * 4);  // distance between the pieces of one sequence
    // (the same in bytes, for uni_piece below)
    unsigned ck_off = ck_off_e * (unsigned)sizeof(real), sq_off = sq_off_e * 2u;
    const unsigned ck_piece = ck_piece_e * (unsigned)sizeof(real);
    int blk = 0;
    // one lean piece (64 sites, full blocks, no warm-up boundary) of a wave whose sequences share their observation
    // row: the piece's codes as two scalar 64-bit words, shifted down one block at a time
    int64_t ck_step_b = ck_step * (int64_t)sizeof(real), eb_step_b = nseq * 2;  // block-to-block distances in bytes ...
    if constexpr (DENSE) asm volatile("" : "+s"(ck_step_b), "+s"(eb_step_b));     // ... kept in SGPRs, not recomputed per block
    auto uni_piece = [&](const uint64_t lo, const uint64_t hi) {
        if constexpr (CKPT) {
            if (A.seg_blocks > 0) {  // segments are whole pieces: a segment can only start with the piece
                if (seg_left == 0) {
                    if (active && rank == 0) *esp = E;
                    esp += nseq;
                    seg_left = A.seg_blocks;
                }
                seg_left -= BPC;
            }
        }
        char* ck_u = (char*)((real*)A.ckpt + (int64_t)blk * ck_step);
        char* eb_u = (char*)(A.eblk + (int64_t)blk * nseq);
        // (two halves of BPC / 2 blocks: the codes of a block are the low bits of ONE 64-bit scalar, shifted down)
#pragma nounroll
        for (int hf = 0; hf < 2; ++hf) {
            uint64_t cw = hf == 0 ? lo : hi;
#pragma nounroll
            for (int bi = 0; bi < BPC / 2; ++bi) {
                // (the offsets pass through an empty asm: hoisted out of the loop as 64-bit values they would be added
                // to the base with a v_lshl_add_u64 per store; seen next to the store they are its 32-bit offset operand)
                asm volatile("" : "+v"(ck_off), "+v"(sq_off));
                if constexpr (CKPT) {
#if !PHK_EXP_NO_CKPT_STORE
#pragma unroll
                    for (int i = 0; i < SPL; ++i)
                        ck_store((real*)(ck_u + (ck_off + (unsigned)(i / 4) * ck_piece + (unsigned)(i % 4) * (unsigned)sizeof(real))), L::get(a, i));
#endif
                    ck_u += ck_step_b;
                }
                const int dE = uni_block((uint32_t)cw & (uint32_t)((uint64_t(1) << (2 * T)) - 1u));
                E += dE;
                if constexpr (CKPT) {
                    *(int16_t*)(eb_u + sq_off) = (int16_t)dE;
                    eb_u += eb_step_b;
                    eb_min = dE < eb_min ? dE : eb_min;
                }
                cw >>= 2 * T;
            }
        }
        blk += BPC;
        if constexpr (CKPT) {
            ckp += (int64_t)BPC * ck_step;
            ebp += (int64_t)BPC * nseq;
        }
    };
    auto lean_piece = [&](const int b) { return b + BPC <= nfull && (blkW < b || blkW >= b + BPC); };
    // (uni2 waves) one full block: `ca` / `cb` are the codes of the wave's two rows as scalars.  Every site takes the
    // structured step on the folded factors; a site that is not hom in one of the two rows multiplies by its row behind a
    // wave-uniform branch on one bit (a folded lane's hom row is exactly 1, so the lanes of the other row lose nothing).
    // At 1 % hets + 1 % missing 96-98 % of the sites take the fall-through: no LDS gather, no multiply.  (Round 4 chose
    // per BLOCK between an emission-free body and the per-lane-code body: 72-85 % of the blocks.)
    auto fold_block = [&](const uint32_t ca, const uint32_t cb) {
        const uint32_t cu = ca | cb;
        const uint32_t nhm = (cu | (cu >> 1)) & 0x55555555u;  // bit 2i: site i is not hom in one of the wave's rows
        const uint32_t mine = rowB ? cb : ca;                   // this lane's codes
#pragma unroll
        for (int i = 0; i < T; ++i) {
            V none[NP];
            real sc;
            [[maybe_unused]] real sum_before = real(0);  // (ONDEMAND: of the state entering the site, for the test behind it)
            if constexpr (ONDEMAND) {
                if (rescale_after<NRM>(i)) lane.template fwd_site_sum<false>(a, none, sum_before);
                else lane.template fwd_site<false>(a, none, sc, false);
            } else {
                lane.template fwd_site<false>(a, none, sc, false);
            }
            if constexpr (FREG) {
                // round 6: the two ratio rows in registers, het / missing lanes multiply under the exec mask behind one
                // wave-uniform bit each (round 5: the lane's row from the LDS table, a round trip a lone wave cannot hide)
#pragma unroll
                for (int h = 0; h < NP; ++h) asm volatile("" : : "v"(rhet[h]), "v"(rmis[h]));  // (a use on the hot path: see bwd_kernel)
                if (__builtin_expect((cu >> (2 * i)) & 1u, 0)) {
                    if (((mine >> (2 * i)) & 3u) == 1u) {
#pragma unroll
                        for (int h = 0; h < NP; ++h) a[h] = a[h] * rhet[h];
                    }
                }
                if (__builtin_expect((cu >> (2 * i + 1)) & 1u, 0)) {
                    if (((mine >> (2 * i)) & 3u) == 2u) {
#pragma unroll
                        for (int h = 0; h < NP; ++h) a[h] = a[h] * rmis[h];
                    }
                }
            } else if (__builtin_expect((nhm >> (2 * i)) & 1u, 0)) {
                V e[NP];
                lane.emis((mine >> (2 * i)) & 3, e);
#pragma unroll
                for (int h = 0; h < NP; ++h) a[h] = a[h] * e[h];
            }
            if (rescale_after<NRM>(i)) {
                if constexpr (ONDEMAND) {
                    lane.template rescale_on_demand<RISK_EXP>(a, sum_before, E, ex_slack);
                } else {
                    const int ex = lane.rescale(a);
                    E += ex;
                    if (NRM > 1) ex_slack = min(ex_slack, ex - RISK_EXP);
                }
            }
#if PHK_FWD_SITE_BARRIER
            __builtin_amdgcn_sched_barrier(0);
#endif
        }
    };
    // (uni2 waves) one lean piece: the codes of the wave's two rows (the same row twice in most waves) as scalars
    auto fold_piece = [&](const uint64_t loA, const uint64_t hiA, const uint64_t loB, const uint64_t hiB) {
        if constexpr (CKPT) {
            if (A.seg_blocks > 0) {  // segments are whole pieces: a segment can only start with the piece
                if (seg_left == 0) {
                    if (active && rank == 0) *esp = E;
                    esp += nseq;
                    seg_left = A.seg_blocks;
                }
                seg_left -= BPC;
            }
        }
        real* ck_u = (real*)A.ckpt + (int64_t)blk * ck_step;
        int16_t* eb_u = A.eblk + (int64_t)blk * nseq;
#pragma nounroll
        for (int hf = 0; hf < 2; ++hf) {
            uint64_t wa = hf == 0 ? loA : hiA, wb = hf == 0 ? loB : hiB;
#pragma nounroll
            for (int bi = 0; bi < BPC / 2; ++bi) {
                if constexpr (CKPT) {
#if !PHK_EXP_NO_CKPT_STORE
#pragma unroll
                    for (int i = 0; i < SPL; ++i) ck_store(&ck_u[ck_off_e + (unsigned)(i / 4) * ck_piece_e + (unsigned)(i % 4)], L::get(a, i));
#endif
                    ck_u += ck_step;
                }
                const int E0 = E;
                const uint32_t ca = (uint32_t)wa & (uint32_t)((uint64_t(1) << (2 * T)) - 1u);
                const uint32_t cb = (uint32_t)wb & (uint32_t)((uint64_t(1) << (2 * T)) - 1u);
                fold_block(ca, cb);
                if constexpr (CKPT) {
                    eb_u[sq_off_e] = (int16_t)(E - E0);
                    eb_u += nseq;
                    eb_min = (E - E0) < eb_min ? (E - E0) : eb_min;
                }
                wa >>= 2 * T;
                wb >>= 2 * T;
            }
        }
        blk += BPC;
        if constexpr (CKPT) {
            ckp += (int64_t)BPC * ck_step;
            ebp += (int64_t)BPC * nseq;
        }
    };
    int budget = A.loop_budget[0];  // (see KArgs::loop_budget; wave-uniform)
    for (int pc = 0; blk < nblk; pc += PPB) {
     if (__builtin_expect(--budget < 0, 0)) break;
     if constexpr (LEAN && FOLD) {
         // uni2 waves read both rows by scalar loads for as long as the pieces are lean (see the one-state-per-lane
         // loop below: no wait for the checkpoint stores; each piece is landed before the next is requested)
         if (uni2 && lean_ok && lean_piece(blk)) {
             const ScalarPieces spA = scalar_pieces(pieces), spB = scalar_pieces_of_lane(pieces, 63);
             [[maybe_unused]] bool ran = false;
#if PHK_FWD_RUN
             // K = 16, one lane per sequence, float32, with checkpoints: the whole run of lean pieces as ONE hand-written instruction
             // sequence (scripts/gen_fwd_asm.py): the do-while below with fold_piece / fold_block inside it, operation for operation --
             // an all-hom block without its eight per-site tests, a mixed block with them, under one register plan; the state's zero
             // pairing and the store addresses are the generator's.  Same bits (tests/test_fwd_run.py).
             if constexpr (sizeof(real) == 4 && K == 16 && R == 1 && T == 8 && NRM == 4 && CKPT && !PHK_KERNEL_MR) {
                 static_assert(ONDEMAND && !FREG && BPC == 8 && NP == 8 && L::EROW == 16 && RISK_EXP == -64 && PHK_CK_NT == 1 && !PHK_EXP_NO_CKPT_STORE &&
                                   !PHK_EXP_NO_BLOCK_RESCALE,
                               "fwd_run_k16r1.inc: the sequence is the body of this configuration");
                 if (A.fwd_run != 0) {
                     auto uni32 = [](uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); };
                     const uint64_t pA = (uint64_t)spA, pB = (uint64_t)spB;
                     const uint64_t cku = (uint64_t)((real*)A.ckpt + (int64_t)blk * ck_step), ebu = (uint64_t)(A.eblk + (int64_t)blk * nseq);
                     const uint64_t ckstep_b = (uint64_t)(ck_step * (int64_t)sizeof(real)), ebstep_b = (uint64_t)(nseq * (int64_t)sizeof(int16_t));
                     const uint32_t fr_pa_lo = uni32((uint32_t)pA), fr_pa_hi = uni32((uint32_t)(pA >> 32));
                     const uint32_t fr_pb_lo = uni32((uint32_t)pB), fr_pb_hi = uni32((uint32_t)(pB >> 32));
                     const uint32_t fr_cku_lo = uni32((uint32_t)cku), fr_cku_hi = uni32((uint32_t)(cku >> 32));
                     const uint32_t fr_ebu_lo = uni32((uint32_t)ebu), fr_ebu_hi = uni32((uint32_t)(ebu >> 32));
                     const uint32_t fr_ckstep_lo = uni32((uint32_t)ckstep_b), fr_ckstep_hi = uni32((uint32_t)(ckstep_b >> 32));
                     const uint32_t fr_ebstep_lo = uni32((uint32_t)ebstep_b), fr_ebstep_hi = uni32((uint32_t)(ebstep_b >> 32));
                     const uint64_t espstep_b = (uint64_t)(nseq * (int64_t)sizeof(int32_t));
                     const uint64_t fr_espstep = ((uint64_t)uni32((uint32_t)(espstep_b >> 32)) << 32) | uni32((uint32_t)espstep_b);
                     const uint64_t fr_act = __ballot(active), fr_rowb = __ballot(rowB);
                     const uint32_t fr_off[4] = {ck_off, ck_off + ck_piece, ck_off + 2u * ck_piece, ck_off + 3u * ck_piece};  // (bytes; < 2^31: lean_ok)
                     const uint32_t fr_sqoff = sq_off, fr_lds = (uint32_t)(uintptr_t)lane.etab;
                     const int fr_npm1 = __builtin_amdgcn_readfirstlane(npieces - 1), fr_nfull = __builtin_amdgcn_readfirstlane(nfull);
                     const int fr_blkw = __builtin_amdgcn_readfirstlane(blkW), fr_segb = __builtin_amdgcn_readfirstlane(A.seg_blocks);
                     const uint32_t fr_thr = uni32(__builtin_bit_cast(uint32_t, real(1) / real(int64_t(1) << PHK_RESCALE_TRIGGER_EXP)));
                     int fr_blk = __builtin_amdgcn_readfirstlane(blk), fr_pc = __builtin_amdgcn_readfirstlane(pc);
                     int fr_budget = __builtin_amdgcn_readfirstlane(budget), fr_segl = __builtin_amdgcn_readfirstlane(seg_left);
                     uint64_t fr_esp = (uint64_t)esp;
                     const int blk0 = fr_blk;
#include "fwd_run_k16r1.inc"
                     blk = fr_blk;
                     pc = fr_pc;
                     budget = fr_budget;
                     seg_left = fr_segl;
                     esp = (int32_t*)fr_esp;
                     ckp += (int64_t)(blk - blk0) * ck_step;
                     ebp += (int64_t)(blk - blk0) * nseq;
                     ran = true;
                 }
             }
#endif
             if (!ran) {
                 PieceWords nA = spA[pc], nB = spB[pc];
                 do {
                     PieceWords cA = nA, cB = nB;
                     asm volatile("" : "+s"(cA.x), "+s"(cA.y), "+s"(cA.z), "+s"(cA.w), "+s"(cB.x), "+s"(cB.y), "+s"(cB.z), "+s"(cB.w) : : "memory");
                     nA = spA[pc + 1 < npieces ? pc + 1 : npieces - 1];
                     nB = spB[pc + 1 < npieces ? pc + 1 : npieces - 1];
                     fold_piece((uint64_t)cA.x | ((uint64_t)cA.y << 32), (uint64_t)cA.z | ((uint64_t)cA.w << 32),
                                (uint64_t)cB.x | ((uint64_t)cB.y << 32), (uint64_t)cB.z | ((uint64_t)cB.w << 32));
                     ++pc;
                 } while (lean_piece(blk) && --budget >= 0);
             }
             if (blk >= nblk || budget < 0) break;
             pnext = pieces[pc < npieces ? pc : npieces - 1];
         }
     }
     if constexpr (LEAN && DENSE && PHK_DENSE_UNI != 0 && PHK_UNI_SLOAD != 0) {
         // Such a wave reads its observation words by SCALAR loads for as long as the pieces are lean: s_load counts
         // in lgkmcnt, so the wait for the piece requested ahead no longer drains the checkpoint stores (vmcnt counts
         // loads and stores alike on gfx9, and the compiler cannot count the stores of a piece through its branches:
         // one store round trip per 64 sites).  No vector load is issued or consumed inside this loop; the piece
         // after it (warm-up boundary, row tail) is requested again for the general path below.
         if (uni && lean_ok && lean_piece(blk)) {
             const ScalarPieces sp = scalar_pieces(pieces);
             PieceWords snext = sp[pc];
             do {
                 PieceWords sc = snext;
                 // land this piece BEFORE the next one is requested: scalar loads return out of order, s_waitcnt
                 // lgkmcnt(0) is the only wait they have, and it would wait for the piece requested ahead as well
                 asm volatile("" : "+s"(sc.x), "+s"(sc.y), "+s"(sc.z), "+s"(sc.w) : : "memory");
                 snext = sp[pc + 1 < npieces ? pc + 1 : npieces - 1];
                 uni_piece((uint64_t)sc.x | ((uint64_t)sc.y << 32), (uint64_t)sc.z | ((uint64_t)sc.w << 32));
                 ++pc;
             } while (lean_piece(blk) && --budget >= 0);
             if (blk >= nblk || budget < 0) break;
             pnext = pieces[pc < npieces ? pc : npieces - 1];
         }
     }
     const uint4 c0 = pnext, c1 = nx1, c2 = nx2, c3 = nx3;
     if constexpr (PPB == 4) {  // one wait for all four: none of them is "maybe in flight" inside the q loop
         asm volatile("" ::"v"(c0.x), "v"(c0.y), "v"(c0.z), "v"(c0.w), "v"(c1.x), "v"(c1.y), "v"(c1.z), "v"(c1.w),
                      "v"(c2.x), "v"(c2.y), "v"(c2.z), "v"(c2.w), "v"(c3.x), "v"(c3.y), "v"(c3.z), "v"(c3.w));
     }
     pnext = pieces[pc + PPB < npieces ? pc + PPB : npieces - 1];
     if constexpr (PPB == 4) {
         nx1 = pieces[pc + 5 < npieces ? pc + 5 : npieces - 1];
         nx2 = pieces[pc + 6 < npieces ? pc + 6 : npieces - 1];
         nx3 = pieces[pc + 7 < npieces ? pc + 7 : npieces - 1];
     }
#pragma nounroll
     for (int q = 0; q < PPB && blk < nblk; ++q) {
      const uint4 pcur = PPB == 1 ? c0 : (q == 0 ? c0 : (q == 1 ? c1 : (q == 2 ? c2 : c3)));
      const int bend = blk + BPC < nblk ? blk + BPC : nblk;
      if constexpr (LEAN) {
          if (lean_ok && lean_piece(blk)) {
              if (DENSE && PHK_DENSE_UNI != 0 && uni) {
                  uni_piece((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)pcur.x) |
                                ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)pcur.y) << 32),
                            (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)pcur.z) |
                                ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)pcur.w) << 32));
                  continue;
              }
              if constexpr (CKPT) {
                  if (A.seg_blocks > 0) {  // segments are whole pieces: a segment can only start with the piece
                      if (seg_left == 0) {
                          if (active && rank == 0) *esp = E;
                          esp += nseq;
                          seg_left = A.seg_blocks;
                      }
                      seg_left -= BPC;
                  }
              }
              real* ck_u = (real*)A.ckpt + (int64_t)blk * ck_step;
              int16_t* eb_u = A.eblk + (int64_t)blk * nseq;
              uint32_t w0 = pcur.x, w1 = pcur.y, w2 = pcur.z, w3 = pcur.w;
#pragma nounroll
              for (int bi = 0; bi < BPC; ++bi) {
                  if constexpr (CKPT) {
#if !PHK_EXP_NO_CKPT_STORE
#pragma unroll
                      for (int i = 0; i < SPL; ++i) ck_store(&ck_u[ck_off_e + (unsigned)(i / 4) * ck_piece_e + (unsigned)(i % 4)], L::get(a, i));
#endif
                      ck_u += ck_step;
                  }
                  const int E0 = E;
                  if constexpr (DENSE) dense_block(w0);
                  else straight_block(w0);
                  if constexpr (CKPT) {
                      eb_u[sq_off_e] = (int16_t)(E - E0);
                      eb_u += nseq;
                      eb_min = (E - E0) < eb_min ? (E - E0) : eb_min;
                  }
                  if constexpr (T == 16) {
                      w0 = w1; w1 = w2; w2 = w3;
                  } else {
                      w0 = __builtin_amdgcn_alignbit(w1, w0, 2 * T);
                      w1 = __builtin_amdgcn_alignbit(w2, w1, 2 * T);
                      w2 = __builtin_amdgcn_alignbit(w3, w2, 2 * T);
                      w3 >>= 2 * T;
                  }
              }
              blk += BPC;
              if constexpr (CKPT) {
                  ckp += (int64_t)BPC * ck_step;
                  ebp += (int64_t)BPC * nseq;
              }
              continue;
          }
      }
      for (int bi = 0; blk < bend; ++blk, ++bi) {
        const int tw = (bi * T) & 15;  // first site of the block inside its word
        const int wsel = (bi * T) >> 4;
        const uint32_t wcur = wsel == 0 ? pcur.x : (wsel == 1 ? pcur.y : (wsel == 2 ? pcur.z : pcur.w));
        if constexpr (CKPT) {
            if (active) {
#pragma unroll
                for (int i = 0; i < SPL; ++i) ck_store(&ckp[L::ck_elem(i, nseq)], L::get(a, i));
            }
            ckp += ck_step;
        }
        const int E0 = E;
        if constexpr (CKPT) {
            if (A.seg_blocks > 0) {
                if (seg_left == 0) {
                    if (active && rank == 0) *esp = E;
                    esp += nseq;
                    seg_left = A.seg_blocks;
                }
                --seg_left;
            }
        }
        const uint32_t codes = wcur >> (2 * tw);
        const bool full = blk < nfull && blk != blkW;  // T sites, no warm-up boundary inside
        const int ns = blk < nfull ? T : tail;
        if (DENSE && full) {
            dense_block(codes);
        } else if (full) {
            // full block, no warm-up boundary inside: one straight-line basic block of T sites, so
            // the scheduler can lift every emission ds_read to the top and overlap sites
#if PHK_EMIS_AHEAD >= 2
            // emission rows requested PHK_EMIS_AHEAD sites ahead (a ring; the indices are constants after
            // unrolling): an LDS round trip is ~300 cycles here, more than the ~280 one site takes
            constexpr int AH = PHK_EMIS_AHEAD < T ? PHK_EMIS_AHEAD : T - 1;
            V ring[AH + 1][NP];
#pragma unroll
            for (int j = 0; j < AH; ++j) lane.emis((codes >> (2 * j)) & 3, ring[j]);
#pragma unroll
            for (int i = 0; i < T; ++i) {
                if (i + AH < T) lane.emis((codes >> (2 * (i + AH))) & 3, ring[(i + AH) % (AH + 1)]);
                real sc;
                const int ex = lane.fwd_site(a, ring[i % (AH + 1)], sc, rescale_after<NRM>(i));
                E += ex;
                if (NRM > 1 && rescale_after<NRM>(i)) ex_slack = min(ex_slack, ex - RISK_EXP);
                __builtin_amdgcn_sched_barrier(0);
            }
#else
            straight_block(codes);
#endif
        } else {
#pragma unroll
            for (int i = 0; i < T; ++i) {
                if (i < ns) {
                    real sc;
                    V e[NP];
                    lane.emis((codes >> (2 * i)) & 3, e);
                    const int ex = lane.fwd_site(a, e, sc, rescale_after<NRM>(i));
                    E += ex;
                    if (NRM > 1 && rescale_after<NRM>(i)) ex_slack = min(ex_slack, ex - RISK_EXP);
                    if (blk == blkW && i == iW) {
                        const double cW = (double)lane.total(a);
                        llW = log(cW) + (double)E * LN2;
                    }
                }
            }
        }
        if constexpr (CKPT) {
            if (active && rank == 0) *ebp = (int16_t)(E - E0);
            ebp += nseq;
            eb_min = (E - E0) < eb_min ? (E - E0) : eb_min;
        }
      }
     }
    }
    if (__builtin_expect(budget < 0, 0)) {  // out of its iteration budget: flag, record, leave (the call has failed)
        report_overrun(A, 1, seq, blk);
        return;
    }
    const double cend = (double)lane.total(a);  // Ltot == 0: sum(pi)
    if (NRM > 1 && active && rank == 0 && A.risk != nullptr &&
        (ex_slack < 0 || !(cend > 0.0)))
        atomicOr(A.risk, FLAG_UNDERFLOW);
    if (active && rank == 0) {
        A.ll[sm.oseq] = log(cend) + (double)E * LN2 - llW;  // (the caller's order: see SeqMap)
        if constexpr (CKPT) {
            A.aux[seq].inv_end = 1.0 / cend;
            A.aux[seq].e_end = E;
            A.aux[seq].eb_min = eb_min;
        }
    }
