// The body of bscan_kernel / bscan_kernel_mr (psmc_kernels.hip), included once per kernel with PHK_KERNEL_MR = false / true: see
// fwd_kernel_body.inc.
    using L = Lane<real, K, R>;
    using V = typename L::V;
    constexpr int SPL = L::SPL, NP = L::NP;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    // the scan's wave priority is a launch argument (phk_api.hip: scan_prio_for): its waves share SIMDs with the forward kernel's
    // (priority PHK_FWD_PRIO), and which of the two kernels should win the issue slots depends on which one the rows make longer
    if (A.scan_prio >= 3) __builtin_amdgcn_s_setprio(3);
    else if (A.scan_prio == 2) __builtin_amdgcn_s_setprio(2);
    else if (A.scan_prio == 1) __builtin_amdgcn_s_setprio(1);
    const int64_t nseq = A.B * A.S;
    const int rank = threadIdx.x & (R - 1);
    // (idle waves leave, lane groups are mapped to sequences as in fwd_kernel: see map_group)
    const SeqMap sm = map_group<real, K, R>(A);
#ifndef PHK_KEEP_IDLE_WAVES
    if (sm.idle_wave) return;
#endif
    const bool active = sm.active;
    const int64_t bb = sm.bb, ss = sm.ss, seq = sm.seq;

    L lane;
    V pi[NP], beta[NP];
    lane.load((const real*)A.params + bb * A.pstride_b + ss * A.pstride_s, rank,
              (real*)smem_raw + (size_t)threadIdx.x * L::ETAB_STRIDE, pi);
    const real* pfb = prefold_block<real>(A, bb, ss);
    const bool fold_seq = lane.try_fold(pfb != nullptr ? pfb + rank * L::SPL : nullptr);  // (float32: the folded model, see Lane::try_fold)
    constexpr bool DENSE = has_dense<real, K, R>() && NRM == 4;  // hom-run operators (see dense16)
    if constexpr (DENSE)
        lane.template load_dense<true>(A.ops_b + (A.pstride_s != 0 ? bb * A.S + ss : bb) * DENSE_OPS_FLOATS, rank, fold_seq,
                                       PHK_KERNEL_MR ? (float*)smem_raw + (size_t)blockDim.x * L::ETAB_STRIDE + (size_t)threadIdx.x * DENSE_Q8_STRIDE : nullptr);
#pragma unroll
    for (int h = 0; h < NP; ++h) beta[h] = splat<real>(real(0));
#pragma unroll
    for (int i = 0; i < SPL; ++i) L::set(beta, i, real(1));
    const uint32_t* words = A.packed + checked_row(A, ss) * A.Lw;
    bool uni = false;  // the wave's sequences share their observation row and the emission ratios exist (see fwd_kernel)
    if constexpr (DENSE && PHK_DENSE_UNI_SCAN != 0) {
        const int ss0 = __builtin_amdgcn_readfirstlane((int)ss);
        uni = __all((int)ss == ss0 && (fold_seq || lane.etab[0] > RATIO_MIN_EMIS0)) != 0;
    }
    int F = 0;
    int f_slack = 1 << 20;  // dense kernel: smallest distance to its threshold of an exponent a rescale removed (see fwd_kernel: ex_slack)
    int hom_run = 0;  // dense kernel: rescale debt (hom sites stepped over since the last rescale; uniform path: + 16 per het / missing site)
    // 32-bit wave-uniform bookkeeping, no division inside the loop (see fwd_kernel)
    const int nw = (int)((A.Ltot + 15) / 16);
    const int seg_words = (int)(seg_sites >> 4);  // segments are whole words (SEG_SITES = 512)
    const int tail = (int)(A.Ltot - (int64_t)(nw - 1) * 16);  // sites in the last word (1..16)
    // the first segment start met from the right: the largest multiple of seg_sites below Ltot
    int sb = (int)((A.Ltot - 1) / seg_sites);            // its segment index (0: none to store)
    int w_store = sb * seg_words - 1;                    // store before processing this word ...
    // 16-byte pieces (4 words) requested one piece ahead; word loop nested in the piece loop (see fwd_kernel)
    const uint4* pieces = (const uint4*)words;
    int w = nw - 1;
    int pc = w >> 2;
    uint4 pnext = pieces[pc > 0 ? pc : 0];
    if constexpr (sizeof(real) == 4 || PHK_EXP_LAND_F64) asm volatile("" ::"v"(pnext.x), "v"(pnext.y), "v"(pnext.z), "v"(pnext.w));  // see fwd_kernel
    // one whole word (16 sites, right to left) of the other layouts: straight-line, next emission row in flight
    auto straight_word = [&](const uint32_t codes) {
        V ec[NP];
        lane.emis(codes >> 30, ec);
#pragma unroll
        for (int j = 15; j >= 0; --j) {
            V en[NP];
            if (j > 0) lane.emis((codes >> (2 * (j - 1))) & 3, en);
            F += lane.bt_site(beta, ec, rescale_after<NRM>(j));
            if (j > 0) {
#pragma unroll
                for (int h = 0; h < NP; ++h) ec[h] = en[h];
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // one whole word (16 sites, right to left) of the one-state-per-lane layout: dense M_h^16 / M_h^8 / M_h^4 /
    // M_h^2 steps where every sequence of the wave is hom over the sites they cover (see fwd_kernel)
    auto dense_word = [&](const uint32_t codes) {
        if constexpr (DENSE) {
            if (PHK_DENSE16 && __all(codes == 0u)) {  // (one rescale per PHK_DENSE_RESCALE_SITES hom sites: see fwd_kernel)
                beta[0][0] = dense16(beta[0][0], lane.D16);
                hom_run += 16;
                if (hom_run >= PHK_DENSE_RESCALE_SITES) {
                    hom_run = 0;
                    const int ex = lane.rescale(beta);
                    F += ex;
                    f_slack = min(f_slack, ex - RISK_EXP_DEFERRED_F32);
                }
                return;
            }
#pragma unroll
            for (int h8 = 1; h8 >= 0; --h8) {
                if (PHK_DENSE8 && __all(((codes >> (16 * h8)) & 0xffffu) == 0u)) {
                    beta[0][0] = dense16(beta[0][0], lane.P[7]);
                    hom_run += 8;
                    if (hom_run >= PHK_DENSE_RESCALE_SITES) {
                        hom_run = 0;
                        const int ex = lane.rescale(beta);
                        F += ex;
                        f_slack = min(f_slack, ex - RISK_EXP_DEFERRED_F32);
                    }
                    continue;
                }
                hom_run = 0;
#pragma unroll
                for (int g = 2 * h8 + 1; g >= 2 * h8; --g) {
                    const uint32_t c4 = (codes >> (8 * g)) & 0xffu;
                    if (__all(c4 == 0u)) {
                        beta[0][0] = dense16(beta[0][0], lane.P[3]);
                    } else {
#pragma unroll
                        for (int hh = 1; hh >= 0; --hh) {
                            const uint32_t c2 = (c4 >> (4 * hh)) & 0xfu;
                            if (__all(c2 == 0u)) {
                                beta[0][0] = dense16(beta[0][0], lane.P[1]);
                            } else {
                                V e[NP];
                                lane.emis(c2 >> 2, e);
                                lane.bt_site(beta, e, false);
                                lane.emis(c2 & 3, e);
                                lane.bt_site(beta, e, false);
                            }
                        }
                    }
                    const int ex = lane.rescale(beta);
                    F += ex;
                    f_slack = min(f_slack, ex - RISK_EXP_F32);
                }
            }
        }
    };
    // One whole word of a wave whose sequences share their observation row (see fwd_kernel, uni_block): right to left,
    // a run is "a het or missing site (multiply by its ratio FIRST: b <- M_h (ratio .* b)), then the hom sites to its
    // left", one dense M_h^n step; the leading run of a word may start with a hom site.
    auto uni_word = [&](const uint32_t rem) {
        if constexpr (DENSE) {
            float x = beta[0][0];
            const int risk_exp = rem != 0u ? RISK_EXP_F32 : RISK_EXP_DEFERRED_F32;  // (as uni_block of fwd_kernel)
            auto resc = [&](float& y) -> int {
                const int ex = lane.rescale1(y);
                F += ex;
                f_slack = min(f_slack, ex - risk_exp);
                return 0;
            };
            if (__builtin_expect(rem == 0u, 1)) {  // all hom
                x = dense16(x, lane.D16);
                hom_run += 16;
            } else {
                hom_run = lane.template half_step<false, PHK_KERNEL_MR>(x, rem >> 16, hom_run, resc);
                if (__builtin_expect(hom_run >= PHK_DENSE_RESCALE_SITES, 0)) hom_run = resc(x);
                hom_run = lane.template half_step<false, PHK_KERNEL_MR>(x, rem & 0xffffu, hom_run, resc);
            }
            if (__builtin_expect(hom_run >= PHK_DENSE_RESCALE_SITES, 0)) hom_run = resc(x);
            beta[0][0] = x;
        }
    };
    // seed of segment sb (beta at site sb * seg_sites) before word w_store is processed
    auto store_seed = [&]() {
        real* dst = (real*)bseg_out + ((int64_t)sb * nseq + seq) * K + rank * SPL;
#pragma unroll
        for (int i = 0; i < SPL; ++i) dst[i] = L::get(beta, i);
        fseg_out[(int64_t)sb * nseq + seq] = F;
        --sb;
        w_store -= seg_words;
    };
    int budget = A.loop_budget[2];  // (see KArgs::loop_budget)
    for (; w >= 0; --pc) {
      if (__builtin_expect(--budget < 0, 0)) break;
      if constexpr (DENSE && PHK_DENSE_LEAN != 0 && PHK_DENSE_UNI_SCAN != 0 && PHK_UNI_SLOAD != 0) {
          // A wave whose sequences share their observation row reads it by scalar loads from here to the row's start
          // (every piece left of the one holding the last word is four whole words): see fwd_kernel.  The four words
          // of a piece, right to left, as the high halves of two 64-bit scalars shifted up.
          if (uni && w == pc * 4 + 3 && w < nw - 1 && (seg_words & 3) == 0) {
              const ScalarPieces sp = scalar_pieces(pieces);
              PieceWords snext = sp[pc];
              do {
                  PieceWords sc = snext;
                  asm volatile("" : "+s"(sc.x), "+s"(sc.y), "+s"(sc.z), "+s"(sc.w) : : "memory");  // (land it before the next request)
                  snext = sp[pc > 0 ? pc - 1 : 0];
                  // a seed is stored before word w_store = sb * seg_words - 1 (-1 when none is left: no test of sb), with
                  // segments of whole pieces always the first word of a piece met from the right: one test per piece
                  if (__builtin_expect(w == w_store, 0)) store_seed();
#pragma nounroll
                  for (int hf = 0; hf < 2; ++hf) {
                      uint64_t cw = hf == 0 ? ((uint64_t)sc.z | ((uint64_t)sc.w << 32)) : ((uint64_t)sc.x | ((uint64_t)sc.y << 32));
#pragma nounroll
                      for (int k = 0; k < 2; ++k, --w) {
                          uint32_t rem = (uint32_t)(cw >> 32);
                          asm volatile("" : "+s"(rem));  // (a 32-bit scalar of its own: "rem == 0" is then s_cmp_eq_u32, not a 64-bit VALU compare of cw)
                          uni_word(rem);
                          cw <<= 32;
                      }
                  }
                  --pc;
              } while (w >= 0 && --budget >= 0);
              break;
          }
      }
      const uint4 pcur = pnext;
      pnext = pieces[pc > 0 ? pc - 1 : 0];
      if constexpr (DENSE ? PHK_DENSE_LEAN != 0 : PHK_FWD_LEAN != 0) {
          // lean path (see fwd_kernel): a piece of four whole words, none of them the row's last (partial)
          // word: the words rotate through one register, the segment-start test is the only one left
          if (w == pc * 4 + 3 && w < nw - 1) {
              if (DENSE && PHK_DENSE_UNI_SCAN != 0 && uni) {
                  uint64_t hi = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)pcur.z) |
                                ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)pcur.w) << 32);
                  uint64_t lo = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)pcur.x) |
                                ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)pcur.y) << 32);
#pragma nounroll
                  for (int k = 0; k < 4; ++k, --w) {
                      if (w == w_store && sb > 0) {  // beta now stands at site (w + 1) * 16 = sb * seg_sites
                          real* dst = (real*)bseg_out + ((int64_t)sb * nseq + seq) * K + rank * SPL;
#pragma unroll
                          for (int i = 0; i < SPL; ++i) dst[i] = L::get(beta, i);
                          fseg_out[(int64_t)sb * nseq + seq] = F;
                          --sb;
                          w_store -= seg_words;
                      }
                      uni_word((uint32_t)(hi >> 32));
                      hi = (hi << 32) | (lo >> 32);
                      lo <<= 32;
                  }
                  continue;
              }
              uint32_t w3 = pcur.w, w2 = pcur.z, w1 = pcur.y, w0 = pcur.x;
#pragma nounroll
              for (int k = 0; k < 4; ++k, --w) {
                  if (w == w_store && sb > 0) {  // beta now stands at site (w + 1) * 16 = sb * seg_sites
                      real* dst = (real*)bseg_out + ((int64_t)sb * nseq + seq) * K + rank * SPL;
#pragma unroll
                      for (int i = 0; i < SPL; ++i) dst[i] = L::get(beta, i);
                      fseg_out[(int64_t)sb * nseq + seq] = F;
                      --sb;
                      w_store -= seg_words;
                  }
                  if constexpr (DENSE) dense_word(w3);
                  else straight_word(w3);
                  w3 = w2; w2 = w1; w1 = w0;
              }
              continue;
          }
      }
      for (const int wlo = pc * 4; w >= wlo; --w) {
        const int wsel = w & 3;
        const uint32_t codes = wsel == 0 ? pcur.x : (wsel == 1 ? pcur.y : (wsel == 2 ? pcur.z : pcur.w));
        if (w == w_store && sb > 0) {  // beta now stands at site (w + 1) * 16 = sb * seg_sites
            if (active) {
                real* dst = (real*)bseg_out + ((int64_t)sb * nseq + seq) * K + rank * SPL;
#pragma unroll
                for (int i = 0; i < SPL; ++i) dst[i] = L::get(beta, i);
                if (rank == 0) fseg_out[(int64_t)sb * nseq + seq] = F;
            }
            --sb;
            w_store -= seg_words;
        }
        const int ns = w == nw - 1 ? tail : 16;
        if (DENSE && ns == 16) {
            dense_word(codes);
        } else if (ns == 16) {
            straight_word(codes);
        } else {
#pragma unroll
            for (int j = 15; j >= 0; --j) {
                if (j < ns) {
                    V e[NP];
                    lane.emis((codes >> (2 * j)) & 3, e);
                    F += lane.bt_site(beta, e, rescale_after<NRM>(j));
                }
            }
        }

      }
    }
    if (__builtin_expect(budget < 0, 0)) {
        report_overrun(A, 4, seq, w);
        return;
    }
    if constexpr (DENSE) {  // the scan's own underflow flag (its seeds feed the segment sweep; see fwd_kernel for the thresholds)
        if (active && rank == 0 && A.risk != nullptr && f_slack < 0) atomicOr(A.risk, FLAG_UNDERFLOW);
    }
