// Body of the halo kernel (conv_kernel_halo.h), included once per kernel: conv_halo_h3 (SP = 0, the dense kernel - its text
// is this file with every `if constexpr (SP != 0)` branch discarded, so its code does not depend on the sibling) and
// conv_halo_ts (SP = 1, 2: tap-sparse).  In scope: TM, TN, WM, WN, PK, NI, MODE, KS, SP and the parameter block `hk`.
// conv_halo_en (EN = 1, "entry NiN"): source 0 is not loaded but computed, x0 = b_in + sum_k w_in[k] elu(u[k]) from the <= 8
// channels of `en.u` - conv_pointwise_small's fp32 chain - and the epilogue's residual is that chain again on the patch's own
// pixels.  In scope then: EN and the parameter block `en` (EntryK); the other kernels see EN = 0 and an `en` nothing reads.
    constexpr bool BF = MODE == 1, F32 = MODE == 2, F16 = MODE == 3;
    constexpr bool ONE = BF || F16;                // one product per operand pair: one LDS image, one weight fragment per 16 columns
    constexpr int CH = HALO_CH, HPITCH = HALO_PP;
    constexpr int CPP = CH / 4;                    // 16-byte fp32 items per halo pixel
    constexpr int LOGC = 3;
    const ConvK& p = hk.c;
    constexpr int BM = 32 * TM * WM;               // 128 output pixels = 8 rows x 16 columns
    constexpr int BN = 32 * TN * WN;
    constexpr int PR = BM / 16;                    // patch rows
    static_assert(BM == 128 && WM * WN * KS == 4, "8x16 pixel patch, 4 waves");
    static_assert(KS == 1 || (WM == 1 && TN == 1 && TM == 4), "K split: every wave owns the whole patch and one 32-column tile");
    extern __shared__ __attribute__((aligned(16))) _Float16 smem_h[];
    const int HP = hk.HH * hk.HW;
    _Float16* Ah = smem_h;                         // [HH][RP]: rows of HW pixels x HPITCH halves (+ row padding)
    _Float16* Al = Ah + hk.HH * hk.RP;
    float* Af = (float*)smem_h;                    // MODE 2: [HH][HW] pixels x 32 fp32 (the same bytes as the two fp16 images)

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = t >> 6;
    FUSG_HSTAMP(0);
    const int wk = wave / (WM * WN);               // K-split index (0 when KS == 1)
    const int wm = (wave % (WM * WN)) / WN, wn = wave % WN;
    const int kc = t & (CPP - 1);

    const int tile = xcd_tile();
    const int mt = fdiv(tile, hk.m_nt);
    const int nt = tile - mt * p.NT;
    int b, t2;
    if (hk.tile_list) { b = mt / hk.tile_count; t2 = hk.tile_list[mt - b * hk.tile_count]; }
    else { b = fdiv(mt, hk.m_tpi); t2 = mt - b * hk.tiles_per_img; }
    const int ty = fdiv(t2, hk.m_tx), tx = t2 - ty * hk.tiles_x;
    const int oy0 = ty * PR, ox0 = tx * 16;

    // ---- halo items of this thread: pixel index inside the source image + validity (same for every chunk)
    int hpix[NI];                                   // iy * W + ix of the (reflected / clamped) source pixel
    int hoff[NI];                                   // LDS offset (halves) of the item
    unsigned hvalid = 0;                            // bit j: item j is inside the image (zero padding)
    unsigned hexist = 0;                            // bit j: item j is a real halo item (j-th pass may overrun HP)
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int item = t + 256 * j;
        const int pix = item >> LOGC;
        hpix[j] = 0;
        hoff[j] = 0;
        if (pix < HP) {
            hexist |= 1u << j;
            const int hy = fdiv(pix, hk.m_hw), hx = pix - hy * hk.HW;
            hoff[j] = F32 ? hy * hk.RP + hx * 32 + ((kc ^ ((hx >> 1) & 7)) << 2)         // floats; 16-byte slot kc swizzled by the column
                          : hy * hk.RP + hx * HPITCH + ((((kc >> 1) ^ (((hx >> 2) & 1) << 1)) << 3) | ((kc & 1) << 2));
            int vy = oy0 - hk.pad_h + hy, vx = ox0 - hk.pad_w + hx;
            bool ok = true;
            if (hk.s2d) {
                // sub-image coordinates; reflection of the full image at -1 / H is a clamp of the sub-image
                int sy = oy0 - 1 + hy, sx = ox0 - 1 + hx;
                const int Hs = p.H >> 1, Ws = p.W >> 1;
                if (p.pad_mode == FUSG_PAD_ZERO) ok = (unsigned)sy < (unsigned)Hs && (unsigned)sx < (unsigned)Ws;
                sy = min(max(sy, 0), Hs - 1); sx = min(max(sx, 0), Ws - 1);
                if (ok) { hvalid |= 1u << j; hpix[j] = 2 * sy * p.W + 2 * sx; }
                continue;
            }
            if (p.pad_mode == FUSG_PAD_REFLECT) {
                vy = vy < 0 ? -vy : (vy >= p.Hv ? 2 * p.Hv - 2 - vy : vy);
                vx = vx < 0 ? -vx : (vx >= p.Wv ? 2 * p.Wv - 2 - vx : vx);
            } else if (p.pad_mode == FUSG_PAD_REPLICATE) {
                vy = min(max(vy, 0), p.Hv - 1);
                vx = min(max(vx, 0), p.Wv - 1);
            } else {
                ok = (unsigned)vy < (unsigned)p.Hv && (unsigned)vx < (unsigned)p.Wv;
            }
            if (ok) { hvalid |= 1u << j; hpix[j] = (vy >> p.ups) * p.W + (vx >> p.ups); }
        }
    }
    const long img_pix0 = (long)b * p.H * p.W;

    // ---- entry NiN: elu(u) of the halo's pixels ([NI * 32 pixels][8] fp32: the overrun items of the last pass read zeros), the NiN's
    // weights [8][C0] and bias [C0] sit in LDS above the two halo images until the epilogue's detour takes the space
    [[maybe_unused]] float* enU = (float*)smem_h + en_lds_floats(hk.HH, hk.RP);
    [[maybe_unused]] float* enW = enU + NI * 32 * 8;
    [[maybe_unused]] float* enB = enW + 8 * p.C0;
    [[maybe_unused]] const bool en_two = en.cin > 4;           // u has a second 16-byte piece per pixel (wave-uniform)
    if constexpr (EN != 0) {
        static_assert(PK == PK_ELU && MODE == 0 && SP == 0 && TN == 1, "entry NiN: the split-fp16 ELU launch, one 32-column tile per wave");
        for (int i = t; i < NI * 64; i += 256) {
            const int pix = i >> 1, hf = i & 1;
            const int hy = fdiv(pix, hk.m_hw), hx = pix - hy * hk.HW;
            const int vy = oy0 - hk.pad_h + hy, vx = ox0 - hk.pad_w + hx;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (pix < HP && (unsigned)vy < (unsigned)p.Hv && (unsigned)vx < (unsigned)p.Wv && (hf == 0 || en_two)) {
                v = *(const f32x4*)(en.u + b * en.usn + vy * en.ush + vx * en.usw + hf * 4);
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = elu1(v[c]);
            }
            *(f32x4*)(enU + i * 4) = v;
        }
        for (int n = t; n < p.C0; n += 256) {
#pragma unroll
            for (int c = 0; c < 8; ++c) enW[c * p.C0 + n] = c < en.cin ? en.w_in[(long)n * en.kpad + c] : 0.f;
            enB[n] = en.b_in[n];
        }
        __syncthreads();
    }
    // x0 of the epilogue's rows (TMx * 32 rows from patch row index `rows0`, 4 columns from ncol_base per lane: epilogue_rows' map)
    [[maybe_unused]] auto en_res = [&](auto tmc, ResRegs<decltype(tmc)::value, 1>& rr, int rows0, int ncol_base) __attribute__((always_inline)) {
        const int n = ncol_base + (lane & 7) * 4;
        f32x4 w[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) w[c] = *(const f32x4*)(enW + c * p.C0 + n);
        const f32x4 bias = *(const f32x4*)(enB + n);
#pragma unroll
        for (int i = 0; i < decltype(tmc)::value; ++i)
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int r = rows0 + i * 32 + it * 8 + (lane >> 3);
                rr.v[i][it] = en_nin(enU + (((r >> 4) + hk.pad_h) * hk.HW + (r & 15) + hk.pad_w) * 8, en_two, w, bias);
            }
    };

    // this wave's weight fragments: tiles (nt*BN/32 + wn*TN + j), j < TN
    constexpr int FPT = BF ? 2 : 4;                            // fragments (1 KiB) per 32-column tile: [ct] or [ct][hi|lo] (MODE 3 reads the hi ones)
    const _Float16* wfr = hk.wfrag + ((long)(nt * (BN / 32) + wn * TN) * FPT * 64 + lane) * 8;
    const long wstep = (long)hk.nt32 * FPT * 64 * 8;          // 16-bit elements per (tap, chunk) slab
    const float vfloor = relu_floor<PK>(p);
    float amax = 0.f;
    const int nchq = p.C0 / CH;                                 // chunks per quadrant (quadrant form)
    const int nch0 = hk.s2d ? 4 * nchq : p.C0 / CH, nch = nch0 + hk.c1k / CH;
    const int nch32 = (p.C0 + hk.c1k) >> 5;
    const int ntaps = hk.kh * hk.kw;
    // tap-sparse: live taps of this wave's phase, in a scalar register (the branches on it are wave-uniform: s_cbranch)
    [[maybe_unused]] unsigned tlive = 0x1ffu;
    if constexpr (SP != 0) {
        static_assert(TN == 1 && MODE != 1 && SP <= 2, "tap-sparse: one 32-column tile per wave, split-fp16 or exact fp32");
        const int n0 = nt * BN + wn * 32, cq = p.Cout >> 2;
        const int ph = (n0 >= cq) + (n0 >= 2 * cq) + (n0 >= 3 * cq);
        constexpr unsigned M0 = tap_sparse_mask(SP, 0), M1 = tap_sparse_mask(SP, 1), M2 = tap_sparse_mask(SP, 2), M3 = tap_sparse_mask(SP, 3);
        tlive = __builtin_amdgcn_readfirstlane(ph == 0 ? M0 : ph == 1 ? M1 : ph == 2 ? M2 : M3);
    }
    [[maybe_unused]] auto live = [&](int tp) __attribute__((always_inline)) { return ((tlive >> tp) & 1u) != 0; };

    if (p.touch_w && gridDim.x <= TOUCH_MAX_WGS) {
        // this wave column's weight slabs: TN * FPT KiB contiguous per (tap, chunk) slab, nslabs slabs wstep apart;
        // the WM waves that share the column take every WM-th group of 64 lines
        constexpr int LPS = TN * FPT * 8;                         // 128-byte lines per slab
        const int nslabs = ntaps * nch32;                         // (quadrant form: the quadrants' taps add up to kh * kw)
        void* dummy = (char*)smem_h + hk.touch_off;
        const _Float16* wcol = hk.wfrag + (long)(nt * (BN / 32) + wn * TN) * FPT * 64 * 8;
        for (int L0 = (wave / WN) * 64; L0 < nslabs * LPS; L0 += WM * KS * 64) {     // the WM * KS waves of a column share the work
            const int L = L0 + lane;
            if (L < nslabs * LPS) {
                const int sl = L / LPS, q = L - sl * LPS;
                l2_touch(wcol + (long)sl * wstep + q * 64, dummy);
            }
        }
    }

    // Staging registers of one chunk's halo.  (Tried in round 3 and dropped: a second set, fetching two chunks ahead on
    // the narrow tiles - conv time of the pass 24.5 -> 25.6 ms: those launches are bound by instruction issue, not by
    // bytes in flight, and the second set only adds instructions.)
    // (every lambda below is always_inline: left to the inliner, the NI >= 10 instantiations kept the staging lambdas as
    // real calls and their register sets went to scratch - 336-368 bytes per lane)
    struct HSet { f32x4 r[NI]; f32x4 sc, sh; };
    HSet hA;
    hA.sc = f32x4{1.f, 1.f, 1.f, 1.f};
    hA.sh = f32x4{0.f, 0.f, 0.f, 0.f};

    // (q, cq) = quadrant and chunk within it of chunk cg in the quadrant form (the callers count them up: no division)
    auto halo_issue = [&](HSet& S, int cg, int q, int cq) __attribute__((always_inline)) {
        if constexpr (EN != 0) {
            // the chunk's 4 channels of this thread's items, computed where the loads would be issued: the chain runs beside the
            // taps of the chunk before; a pixel outside the image is conv A's zero padding, not NiN(0) + bias
            const int n0 = cg * CH + kc * 4;
            f32x4 w[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) w[c] = *(const f32x4*)(enW + c * p.C0 + n0);
            const f32x4 bias = *(const f32x4*)(enB + n0);
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const f32x4 v = en_nin(enU + ((t + 256 * j) >> 3) * 8, en_two, w, bias);
                S.r[j] = ((hvalid >> j) & 1u) ? v : f32x4{0.f, 0.f, 0.f, 0.f};
            }
            return;
        }
        const bool s1 = cg >= nch0;
        const float* base = s1 ? p.src1 : p.src0;
        const int Cs = s1 ? p.Cs1 : p.Cs0;
        int coff = (s1 ? cg - nch0 : cg) * CH + kc * 4;
        long qpix = img_pix0;
        if (hk.s2d) { coff = cq * CH + kc * 4; qpix += (q >> 1) * p.W + (q & 1); }
        if (PK == PK_AFFINE) {
            const long o = (long)b * p.pre_bstride + (s1 ? p.C0 : 0) + coff;
            S.sc = *(const f32x4*)(p.pre_scale + o);
            S.sh = *(const f32x4*)(p.pre_shift + o);
        }
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const float* ptr = base + (qpix + hpix[j]) * Cs + coff;
            if (PK != PK_AFFINE) ptr = ((hvalid >> j) & 1u) ? ptr : p.zeros;
            S.r[j] = *(const f32x4*)ptr;
        }
    };
    auto halo_commit = [&](const HSet& S) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            f32x4 v = S.r[j];
            pre_apply<PK>(v, S.sc, S.sh, (hvalid >> j) & 1u);
            if constexpr (F32) {
                // (only a fused ReLU clamps: fmaxf(NaN, -inf) would turn a NaN into -inf, and a NaN must reach the output)
                if (vfloor == 0.f) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) v[c] = __builtin_fmaxf(v[c], 0.f);
                }
                if ((hexist >> j) & 1u) *(f32x4*)(Af + hoff[j]) = v;
            } else if constexpr (BF) {
                if (vfloor == 0.f) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) v[c] = __builtin_fmaxf(v[c], 0.f);
                }
                const bf4 hb = __builtin_convertvector(v, bf4);
                if ((hexist >> j) & 1u) *(bf4*)(Ah + hoff[j]) = hb;
            } else if constexpr (F16) {
                // MODE 1's NaN rule (fmaxf under a fused ReLU, propagation elsewhere); the split's amax, taken after the floor
                if (vfloor == 0.f) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) v[c] = __builtin_fmaxf(v[c], 0.f);
                }
                asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(amax) : "v"(v[0]), "v"(v[1]));
                asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(amax) : "v"(v[2]), "v"(v[3]));
                const h4 hh = __builtin_convertvector(v, h4);      // v_cvt_f16_f32: round to nearest, ties to even
                if ((hexist >> j) & 1u) *(h4*)(Ah + hoff[j]) = hh;
            } else {
                h4 hi, lo;
                if constexpr (PK == PK_ELU) split4<false>(v, vfloor, hi, lo, amax); else split4(v, vfloor, hi, lo, amax);
                if ((hexist >> j) & 1u) {
                    *(h4*)(Ah + hoff[j]) = hi;
                    *(h4*)(Al + hoff[j]) = lo;
                }
            }
        }
    };
    struct BFrag { h8 f[TN][2][ONE ? 1 : 2]; };       // [32-column tile][16-column half][hi, lo] (bf16, single-pass fp16: one fragment)
    BFrag bfA, bfB;
    auto b_load = [&](BFrag& F, const _Float16* base) __attribute__((always_inline)) {            // base: this wave column's part of one (tap, chunk) slab
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int hl = 0; hl < (ONE ? 1 : 2); ++hl)
                    F.f[j][ct][hl] = *(const h8*)(base + ((j * 2 + ct) * (BF ? 1 : 2) + hl) * 512);
    };

    f32x4 acc[2 * TM][2 * TN];                        // [patch row of the wave][16-column group]
#pragma unroll
    for (int i = 0; i < 2 * TM; ++i)
#pragma unroll
        for (int j = 0; j < 2 * TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // row group i of the wave (16 output pixels) = patch row wm*TM*2 + i; lane l reads pixel l & 15 of it
    int abase[2 * TM];
#pragma unroll
    for (int i = 0; i < 2 * TM; ++i) abase[i] = (wm * TM * 2 + i) * hk.RP;
    auto compute = [&](int dyp, int dxp, const BFrag& F) __attribute__((always_inline)) {          // (dyp, dxp): halo pixel offset of the tap
        const int hx = (lane & 15) + dxp;
        const int toff = dyp * hk.RP + hx * HPITCH + (((lane >> 4) ^ (((hx >> 2) & 1) << 1)) << 3);
        if constexpr (F32) {
            const int sw = (hx >> 1) & 7, g = lane >> 4;
            const int tf = dyp * hk.RP + hx * 32;
            f32x4 a0[2 * TM], a1[2 * TM];
#pragma unroll
            for (int i = 0; i < 2 * TM; ++i) {
                a0[i] = *(const f32x4*)(Af + abase[i] + tf + ((g ^ sw) << 2));
                a1[i] = *(const f32x4*)(Af + abase[i] + tf + (((g + 4) ^ sw) << 2));
            }
            // instruction-major order: consecutive MFMAs write different accumulators (40-cycle dependent latency)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < 2 * TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
#pragma unroll
                            for (int ct = 0; ct < 2; ++ct) {
                                const f32x4 bv = __builtin_bit_cast(f32x4, F.f[j][ct][h]);
                                acc[i][2 * j + ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(h ? a1[i][e] : a0[i][e], bv[e], acc[i][2 * j + ct], 0, 0, 0);
                            }
        } else if constexpr (BF) {
            bf8 ab[2 * TM];
#pragma unroll
            for (int i = 0; i < 2 * TM; ++i) ab[i] = *(const bf8*)(Ah + abase[i] + toff);
#pragma unroll
            for (int i = 0; i < 2 * TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct)
                        acc[i][2 * j + ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ab[i], __builtin_bit_cast(bf8, F.f[j][ct][0]),
                                                                                       acc[i][2 * j + ct], 0, 0, 0);
        } else if constexpr (F16) {
            h8 ah[2 * TM];
#pragma unroll
            for (int i = 0; i < 2 * TM; ++i) ah[i] = *(const h8*)(Ah + abase[i] + toff);
#pragma unroll
            for (int i = 0; i < 2 * TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct)
                        acc[i][2 * j + ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], F.f[j][ct][0], acc[i][2 * j + ct], 0, 0, 0);
        } else {
            h8 ah[2 * TM], al[2 * TM], bs[TN][2];
#pragma unroll
            for (int i = 0; i < 2 * TM; ++i) {
                ah[i] = *(const h8*)(Ah + abase[i] + toff);
                al[i] = *(const h8*)(Al + abase[i] + toff);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) bs[j][ct] = scale_m11(F.f[j][ct][0]);   // wh * 2^-11: B operand of the al' term
            // term-major order: consecutive MFMAs write different accumulators (a dependent chain on one accumulator
            // stalls the issue)
#pragma unroll
            for (int term = 0; term < 3; ++term)
#pragma unroll
                for (int i = 0; i < 2 * TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int ct = 0; ct < 2; ++ct)
                            acc[i][2 * j + ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                                term == 2 ? al[i] : ah[i], term == 0 ? F.f[j][ct][0] : term == 1 ? F.f[j][ct][1] : bs[j][ct],
                                acc[i][2 * j + ct], 0, 0, 0);
        }
    };

    // Step bookkeeping without divisions: a step is (chunk, tap); the launch walks chunk-major.  Three cursors - the
    // step being computed, the step whose weights are being fetched (one ahead) and the chunk whose halo is being
    // fetched - each counted up with its quadrant / chunk-in-quadrant (quadrant form) or (ky, kx) (dense tap grid).
    // The weight slab of (tap, chunk) is tap_global * nch32 + chunk32: consecutive taps of a chunk are `tapstride` apart.
    // (Round 2 derived all of this per step with integer divisions: ~350 mostly scalar instructions per step next to 12
    // MFMAs on the 32-column tile - PMC: those launches spent 36 % of their wave cycles issuing and 29 % stalled on issue
    // at an MFMA-pipe busy of 0.22 - 0.30.)
    const long tapstride = (long)nch32 * wstep;
    const int s2d = hk.s2d;
    // computed step
    int cg = 0, tap = 0, ky = 0, kx = 0, qc = 0, cqc = 0, ntc = s2d ? hk.qtaps[0] : ntaps;
    // fetched step (weights)
    int cgn = 0, tapn = 0, qn = 0, cqn = 0, ntn = ntc;
    const _Float16* wnext = wfr + (long)(s2d ? hk.qwoff[0] : 0) * tapstride;
    // fetched chunk (halo)
    int qh = 0, cqh = 0;
    auto next_halo_chunk = [&]() { if (s2d && ++cqh == nchq) { cqh = 0; ++qh; } };

    // weight cursor -> the next (chunk, tap) step
    auto advance_w = [&]() __attribute__((always_inline)) {
        wnext += tapstride;
        if (++tapn == ntn) {
            tapn = 0;
            ++cgn;
            if (s2d) {
                if (++cqn == nchq) { cqn = 0; ++qn; }
                ntn = hk.qtaps[qn & 3];
                wnext = wfr + (long)hk.qwoff[qn & 3] * tapstride + (long)cqn * wstep;
            } else {
                wnext = wfr + (long)cgn * wstep;
            }
        }
    };

    if constexpr (KS > 1) {
        // ---- K split over the waves: this wave's steps are the taps wk, wk + KS, ... of every chunk (dense tap grid only)
        auto wptr = [&](int cgx, int tapx) __attribute__((always_inline)) { return wfr + (long)tapx * tapstride + (long)cgx * wstep; };
        halo_issue(hA, 0, 0, 0);
        if constexpr (SP != 0) { if (wk < ntaps && live(wk)) b_load(bfA, wptr(0, wk)); } else
        if (wk < ntaps) b_load(bfA, wptr(0, wk));
        halo_commit(hA);
        __syncthreads();
        bool odd = false;
        for (int cgx = 0; cgx < nch; ++cgx) {
            if (cgx + 1 < nch) halo_issue(hA, cgx + 1, 0, 0);         // in flight during this chunk's taps
            int kyx = 0, kxx = wk;
            while (kxx >= hk.kw) { kxx -= hk.kw; ++kyx; }
            for (int tapx = wk; tapx < ntaps; tapx += KS) {
                int ntap = tapx + KS, ncg = cgx;                       // this wave's next step: its weights are fetched now
                if (ntap >= ntaps) { ntap = wk; ++ncg; }
                const _Float16* wn_ptr = wptr(ncg, ntap);
                if constexpr (SP != 0) {
                    if (!odd) { if (ncg < nch && live(ntap)) b_load(bfB, wn_ptr); if (live(tapx)) compute(kyx * hk.dil, kxx * hk.dil, bfA); }
                    else { if (ncg < nch && live(ntap)) b_load(bfA, wn_ptr); if (live(tapx)) compute(kyx * hk.dil, kxx * hk.dil, bfB); }
                } else {
                if (!odd) { if (ncg < nch) b_load(bfB, wn_ptr); compute(kyx * hk.dil, kxx * hk.dil, bfA); }
                else { if (ncg < nch) b_load(bfA, wn_ptr); compute(kyx * hk.dil, kxx * hk.dil, bfB); }
                }
                odd = !odd;
                kxx += KS;
                while (kxx >= hk.kw) { kxx -= hk.kw; ++kyx; }
            }
            if (cgx + 1 < nch) {
                __syncthreads();                                       // every wave is done with the old halo
                halo_commit(hA);
                __syncthreads();
            }
        }
    } else if constexpr (CM != 0) {
    // ---- column-major taps (dense 3x3, dil 1, split-fp16, the wave owns all eight patch rows): a step is a tap COLUMN of a
    // chunk.  Its ten halo-row fragments (hi, lo) at column shift kx are read once; row group i of tap ky uses fragment i + ky.
    // Weights: as in the tap-major loop one tap ahead through bfA / bfB - a column is three taps, so the two sets change roles
    // from one column to the next.  Slab of (ky, kx, chunk) = (3 ky + kx) * tapstride + chunk * wstep: the packed layout's.
    static_assert(TM == 4 && WM == 1 && KS == 1 && SP == 0 && MODE == 0, "column-major taps: the split-fp16 M-whole wide tile");
    halo_issue(hA, 0, 0, 0);
    b_load(bfA, wfr);
    halo_commit(hA);
    __syncthreads();
    int cgc = 0, kxc = 0;
    // The fragments live in eight register slots, halo row r in slot r % 8: row 0 is dead after the ky = 0 tap and row 1 after
    // the ky = 1 tap, so rows 8 and 9 take their slots - the A operands keep the 64 registers of the tap-major loop
    // (DESIGN.md 4.1g: resource figures, and the ten-slot form that was dropped).
    auto tap_mfma = [&](auto kyc, const h8 (&ah)[8], const h8 (&al)[8], const BFrag& F) __attribute__((always_inline)) {
        constexpr int KY = decltype(kyc)::value;
        h8 bs[TN][2];
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) bs[j][ct] = scale_m11(F.f[j][ct][0]);       // wh * 2^-11: B operand of the al' term
        // term-major order, as in compute()
#pragma unroll
        for (int term = 0; term < 3; ++term)
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct)
                        acc[i][2 * j + ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                            term == 2 ? al[(i + KY) & 7] : ah[(i + KY) & 7], term == 0 ? F.f[j][ct][0] : term == 1 ? F.f[j][ct][1] : bs[j][ct],
                            acc[i][2 * j + ct], 0, 0, 0);
    };
    auto one_column = [&](BFrag& F0, BFrag& F1) __attribute__((always_inline)) {      // F0: holds the column's ky = 0 weights
        if (kxc == 0) {
            FUSG_HSTAMP(1 + 3 * cgc);
            if (cgc + 1 < nch) halo_issue(hA, cgc + 1, 0, 0);      // in flight during all taps of this chunk
        }
        const _Float16* wcol = wfr + (long)kxc * tapstride + (long)cgc * wstep;     // slab (ky 0, kxc) of this chunk
        b_load(F1, wcol + 3 * tapstride);
        const int hx = (lane & 15) + kxc;
        const int toff = hx * HPITCH + (((lane >> 4) ^ (((hx >> 2) & 1) << 1)) << 3);
        h8 ah[8], al[8];
        auto a_row = [&](auto slotc, int r) __attribute__((always_inline)) {        // halo row r -> slot r % 8
            ah[decltype(slotc)::value] = *(const h8*)(Ah + r * hk.RP + toff);
            al[decltype(slotc)::value] = *(const h8*)(Al + r * hk.RP + toff);
        };
        a_row(std::integral_constant<int, 0>{}, 0); a_row(std::integral_constant<int, 1>{}, 1);
        a_row(std::integral_constant<int, 2>{}, 2); a_row(std::integral_constant<int, 3>{}, 3);
        a_row(std::integral_constant<int, 4>{}, 4); a_row(std::integral_constant<int, 5>{}, 5);
        a_row(std::integral_constant<int, 6>{}, 6); a_row(std::integral_constant<int, 7>{}, 7);
        tap_mfma(std::integral_constant<int, 0>{}, ah, al, F0);
        // (the barriers keep the scheduler from hoisting the two late rows above the tap that frees their slots: DESIGN.md 4.1g)
        __builtin_amdgcn_sched_barrier(0);
        a_row(std::integral_constant<int, 0>{}, 8);
        b_load(F0, wcol + 6 * tapstride);
        tap_mfma(std::integral_constant<int, 1>{}, ah, al, F1);
        __builtin_amdgcn_sched_barrier(0);
        a_row(std::integral_constant<int, 1>{}, 9);
        // the next column's first tap: (ky 0, kxc + 1) of this chunk, or tap 0 of the next chunk
        if (kxc < 2) b_load(F1, wcol + tapstride);
        else if (cgc + 1 < nch) b_load(F1, wfr + (long)(cgc + 1) * wstep);
        tap_mfma(std::integral_constant<int, 2>{}, ah, al, F0);
        if (++kxc == 3) {
            FUSG_HSTAMP(2 + 3 * cgc);
            kxc = 0;
            if (++cgc < nch) {
                __syncthreads();                                   // every wave is done with the old halo
                halo_commit(hA);
                __syncthreads();
            }
            FUSG_HSTAMP(3 * cgc);
        }
    };
    for (;;) {
        one_column(bfA, bfB);
        if (cgc >= nch) break;
        one_column(bfB, bfA);
        if (cgc >= nch) break;
    }
    } else {
    // ---- prologue: halo of chunk 0 and the first weight fragments
    // (Tried in round 3 and left off: weights TWO steps ahead through a ring of three fragment sets for the short steps -
    // bf16 mode, 16 MFMAs = 256 cycles per step, and the narrow split-fp16 tiles, 12 - 24 MFMAs.  Their waves spend 52 % /
    // 35 - 38 % of their cycles in s_waitcnt (profiles/r03_stalls_bf16_halo_256.txt, r03_pmc_narrow_layers.txt), yet the
    // longer lead made both slower: bf16 leg conv 18.15 -> 18.6 ms, f16x3 leg 24.6 -> 25.2 ms.)
    halo_issue(hA, 0, 0, 0);
    if constexpr (SP != 0) { if (live(0)) b_load(bfA, wnext); } else
    b_load(bfA, wnext);
    halo_commit(hA);
    __syncthreads();
    auto one_step = [&](const BFrag& use, BFrag& fill) __attribute__((always_inline)) {
        if (tap == 0) FUSG_HSTAMP(1 + 3 * cg);
        if (cg == 1) FUSG_HSTAMP(30 + tap);                        // (diagnostic: every tap of the second chunk)
        if (tap == 0 && cg + 1 < nch) {                            // in flight during all taps of this chunk
            next_halo_chunk();
            halo_issue(hA, cg + 1, qh, cqh);
        }
        if (cg == 1 && tap < 2 && nch <= 6) FUSG_HSTAMP(20 + 4 * tap);   // (slots 20.. belong to the chunk stamps of deeper layers)
        advance_w();                                               // the step fetched now: one ahead
        if constexpr (SP != 0) { if (cgn < nch && live(tapn)) b_load(fill, wnext); } else
        if (cgn < nch) b_load(fill, wnext);
        if (cg == 1 && tap < 2 && nch <= 6) FUSG_HSTAMP(21 + 4 * tap);
        int dyp = ky * hk.dil, dxp = kx * hk.dil;                  // halo pixel offset of the tap
        if (s2d) { dyp = hk.qtdy[qc & 3][tap]; dxp = hk.qtdx[qc & 3][tap]; }
        if constexpr (SP != 0) { if (live(tap)) compute(dyp, dxp, use); } else
        compute(dyp, dxp, use);
        if (cg == 1 && tap < 2 && nch <= 6) FUSG_HSTAMP(22 + 4 * tap);
        ++tap;
        if (++kx == hk.kw) { kx = 0; ++ky; }
        if (tap == ntc) {
            FUSG_HSTAMP(2 + 3 * cg);
            tap = 0; ky = 0; kx = 0;
            if (s2d) { if (++cqc == nchq) { cqc = 0; ++qc; } ntc = hk.qtaps[qc & 3]; }
            if (++cg < nch) {
                __syncthreads();                                   // every wave is done with the old halo
                halo_commit(hA);
                __syncthreads();
            }
            FUSG_HSTAMP(3 * cg);
        }
    };
    for (;;) {
        one_step(bfA, bfB);
        if (cg >= nch) break;
        one_step(bfB, bfA);
        if (cg >= nch) break;
    }

    }

    if constexpr (!BF && !F32) report_range(p, amax);
    if constexpr (KS > 1) {
        // ---- K split: partial tiles -> LDS ([wave][128 rows][32 columns] fp32, over the halo images), summed in wave order by
        // the wave that finishes those rows: wave (wk, wn) takes rows 128 / KS * wk ... of column tile wn
        constexpr int RW = 128 / KS, TME = RW / 32;
        [[maybe_unused]] ResRegs<TME, 1> rrk;                          // entry NiN: x0 of the rows this wave finishes, while its LDS is alive
        if constexpr (EN != 0) en_res(std::integral_constant<int, TME>{}, rrk, RW * wk, nt * BN + wn * 32);
        __syncthreads();                                               // every wave is done with the halo images
        float* slabs = (float*)smem_h;
        float* mine = slabs + wave * (128 * 32);
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) mine[(i * 16 + (lane >> 4) * 4 + r) * 32 + j * 16 + (lane & 15)] = acc[i][j][r];
        __syncthreads();
        const int rows0 = RW * wk;
        float* dstw = slabs + wn * (128 * 32) + rows0 * 32;           // column wn's slab of K-split 0: the sum lands here
        for (int e = lane; e < RW * 8; e += 64) {                      // RW rows x 8 float4
            f32x4 sum = *(const f32x4*)(dstw + e * 4);
#pragma unroll
            for (int k2 = 1; k2 < KS; ++k2) sum += *(const f32x4*)(slabs + (k2 * WN + wn) * (128 * 32) + rows0 * 32 + e * 4);
            *(f32x4*)(dstw + e * 4) = sum;
        }
        auto pixk = [&](int row, PixOff& po) {
            const int rr = rows0 + row;
            pix_offsets_yx(p, b, oy0 + (rr >> 4), ox0 + (rr & 15), po);
            return true;
        };
        auto statk = [&](int i) -> float* {
            return p.stats + ((long)b * p.stats_slots + t2 * 4 + (rows0 >> 5) + i) * p.Cout * 2;
        };
        if (p.vec_epi) {
            ResRegs<TME, 1> none;
            if constexpr (EN != 0) epilogue_rows<TME, 1>(p, dstw, lane, nt * BN + wn * 32, pixk, statk, rrk, true); else
            epilogue_rows<TME, 1>(p, dstw, lane, nt * BN + wn * 32, pixk, statk, none, false);
        } else {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int e = lane; e < RW * 32; e += 64) {                 // scalar path: one (row, column) per lane and pass
                const int row = e >> 5, n = nt * BN + wn * 32 + (e & 31);
                if (n >= p.Cout) continue;
                PixOff po, co;
                pixk(row, po);
                chan_offsets(p, n, co);
                epi_store(p, po, co, p.bias[n], p.wscale ? p.wscale[n] : 1.f, dstw[e]);
            }
        }
        return;
    }
    // ---------------------------------------------------------------- epilogue
    auto pixfn = [&](int row, PixOff& po) {
        const int rr = wm * TM * 32 + row;
        pix_offsets_yx(p, b, oy0 + (rr >> 4), ox0 + (rr & 15), po);
        return true;
    };
    auto statfn = [&](int i) -> float* {                       // slot = (patch index, 32-row group of the patch)
        return p.stats + ((long)b * p.stats_slots + t2 * (BM / 32) + ((wm * TM * 32) >> 5) + i) * p.Cout * 2;
    };
    if (p.vec_epi) {
        if constexpr (TM >= 4 && halo_bf16_dense(TM, WM, PK, NI, MODE, KS)) {
            // the wave's tile (TM * 32 rows) leaves in two halves through a wave-private LDS region of half the size (64 KiB per
            // workgroup instead of 128: two workgroups still share a CU); residuals are read in the pass, not prefetched
            // (the prefetch set would be 128 more registers)
            constexpr int TH = TM / 2;
            __syncthreads();
            float* wlds = (float*)smem_h + wave * (TH * 32 * TN * 32);
            ResRegs<TH, TN> none;
            auto do_half = [&](auto halfc) __attribute__((always_inline)) {
                constexpr int half = decltype(halfc)::value;           // compile-time: the accumulators stay in registers
                f32x4 sub[2 * TH][2 * TN];
#pragma unroll
                for (int i = 0; i < 2 * TH; ++i)
#pragma unroll
                    for (int j = 0; j < 2 * TN; ++j) sub[i][j] = acc[half * 2 * TH + i][j];
                auto pixh = [&](int row, PixOff& po) { return pixfn(half * TH * 32 + row, po); };
                auto stath = [&](int i) -> float* { return statfn(half * TH + i); };
                epilogue_vec16<TH, TN>(p, wlds, sub, lane, nt * BN + wn * TN * 32, pixh, stath, none, false);
            };
            do_half(std::integral_constant<int, 0>{});
            do_half(std::integral_constant<int, 1>{});
            return;
        } else {
        ResRegs<TM, TN> rr;
        const bool pre = EN != 0 || p.res0 != nullptr;
        if constexpr (EN != 0) en_res(std::integral_constant<int, TM>{}, rr, wm * TM * 32, nt * BN + wn * TN * 32); else
        if (pre) res_prefetch<TM, TN>(p, lane, nt * BN + wn * TN * 32, pixfn, rr);     // in flight across the barrier and the LDS detour
        __syncthreads();
        float* wlds = (float*)smem_h + wave * (TM * 32 * TN * 32);
        epilogue_vec16<TM, TN>(p, wlds, acc, lane, nt * BN + wn * TN * 32, pixfn, statfn, rr, pre);
        return;
        }
    }
#pragma unroll
    for (int j = 0; j < 2 * TN; ++j) {                     // C/D map of the 16x16 tile: col = lane & 15, row = 4 (lane >> 4) + reg
        const int n = nt * BN + wn * TN * 32 + j * 16 + (lane & 15);
        if (n >= p.Cout) continue;
        PixOff co;
        chan_offsets(p, n, co);
        const float bias = p.bias[n], wsc = p.wscale ? p.wscale[n] : 1.f;
#pragma unroll
        for (int i = 0; i < 2 * TM; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wm * TM * 32 + i * 16 + (lane >> 4) * 4 + r;
                PixOff po;
                pix_offsets_yx(p, b, oy0 + (row >> 4), ox0 + (row & 15), po);
                epi_store(p, po, co, bias, wsc, acc[i][j][r]);
            }
    }
