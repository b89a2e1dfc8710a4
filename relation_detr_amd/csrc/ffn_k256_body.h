// Body of the feed-forward kernels of ffn.hip, included once per kernel (textually, so that the inference kernels compile to the
// code they had before the training variants existed: wrapped in a function the same statements allocate registers differently).
// The including kernel provides, as parameters or constants:
//   LN, MODE, x, ldx, packed, b1, b2, M, F, out, ldo, dbg_arg, gamma, beta, eps, pos, ldp, out2, ldo2, hid, ldh, dhid, ldd
// and, for fp32 at either end of the block (the mixed-precision training kernels; false / null everywhere else):
//   XF32: the rows are read from xf (float, ldx) instead of x, rounded to bf16 (RNE) and also stored as xlp [M, 256] (ldxl)
//   DXF32: the accumulators are stored unrounded to outf (float, ldo) instead of out
#ifdef RDETR_DEV
    const int dbg = dbg_arg;                 // development builds: component-timing mask (1 no weight stream, 2 no barrier, 4 / 8 no GEMM 2 / 1,
                                             // 16 no activation arithmetic: the GEMM 1 accumulators are only packed); lumped order
#else
    constexpr int dbg = 0;                   // product build: no branches inside the MFMA loop (they end the scheduling regions)
#endif
    extern __shared__ __attribute__((aligned(16))) unsigned char ffn_lds[];
    float *b1l = reinterpret_cast<float *>(ffn_lds + 2 * kFfnBufBytes);      // [F]
    float *b2l = b1l + F;                                                     // [256]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, g = lane >> 4;
    if constexpr (MODE != kFfnBwd) {
        for (int i = tid; i < F; i += kFfnThreads) b1l[i] = bf16_bits_to_f32(b1[i]);
        if (tid < kFfnK) b2l[tid] = bf16_bits_to_f32(b2[tid]);
    }
    float *gml = b2l + kFfnK, *btl = gml + kFfnK;                             // LayerNorm weight / bias (gamma != nullptr)
    if (LN && tid < kFfnK) {
        gml[tid] = bf16_bits_to_f32(gamma[tid]);
        btl[tid] = bf16_bits_to_f32(beta[tid]);
    }

    // LDS-DMA of chunk c into buffer c & 1: the chunk's 64 fragments of 1 KiB are one contiguous 64-KiB slab of the PACKED
    // weights (ffn_pack_kernel below), 8 instructions per wave, each a fully coalesced 1-KiB read
    const int nchunks = F / kFfnHC;
    auto issue_piece = [&](int c, int into, int i) __attribute__((always_inline)) {     // piece i of chunk c into buffer `into`
        const unsigned buf = (unsigned)(into * kFfnBufBytes);
        const unsigned char *slab = reinterpret_cast<const unsigned char *>(packed) + (size_t)c * kFfnBufBytes;
        const unsigned lane_off = (unsigned)lane * 16u;
        const int f = wave * 8 + i;                                           // uniform
        const unsigned m0v = buf + (unsigned)f * 1024u;
        const unsigned char *src = slab + f * 1024;
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" : : "s"(m0v), "v"(lane_off), "s"(src) : "memory", "m0");
    };
    auto issue_chunk = [&](int c) {
#pragma unroll
        for (int i = 0; i < 8; ++i) issue_piece(c, c & 1, i);
    };

    __amdgpu_buffer_rsrc_t hrs, drs;                                          // H, dH: up to the end of the last row's F columns
    if constexpr (MODE != kFfnInfer) hrs = __builtin_amdgcn_make_buffer_rsrc(hid, 0, (int)(((M - 1) * ldh + F) * 2), 0x00020000);
    if constexpr (MODE == kFfnBwd) drs = __builtin_amdgcn_make_buffer_rsrc(dhid, 0, (int)(((M - 1) * ldd + F) * 2), 0x00020000);
    // byte offset of lane (row col, columns 8 g ..) inside a 16-row block of leading dimension ld2 / 2, or kFfnNoRow past the last
    // row.  Recomputed from the thread id where it is used (the empty asm keeps it from being hoisted): the chunk loop has no
    // register to hold it in
    auto slot = [&](unsigned ld2, int rows_left) __attribute__((always_inline)) -> unsigned {
        unsigned lv = (unsigned)tid;
        asm volatile("" : "+v"(lv));
        const unsigned cv = lv & 15u;
        return (int)cv < rows_left ? cv * ld2 + (lv & 48u) : kFfnNoRow;
    };
    const unsigned ldh2 = (unsigned)(ldh * 2), ldd2 = (unsigned)(ldd * 2);

    const long long ntiles = (M + kFfnWaves * kFfnRows - 1) / (kFfnWaves * kFfnRows);
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long row_a = (tile * kFfnWaves + wave) * kFfnRows + col, row_b = row_a + 16;
        u32x4 xr[2][8];                                                       // X^T fragments: B operand of GEMM 1, all of K
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            if constexpr (XF32) {
                // 8 floats where the bf16 kernel loads 8 bf16: rounded into the same packed registers, which are also stored -- the
                // bf16 copy of x the weight gradient dW1 = dH^T x reads (autocast would write it in a pass of its own)
                const long long rows2[2] = {row_a, row_b};
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    xr[cb][s] = u32x4{0u, 0u, 0u, 0u};
                    if (rows2[cb] < M) {
                        const float *src = xf + rows2[cb] * ldx + 32 * s + 8 * g;
                        const f32x4 lo = *reinterpret_cast<const f32x4 *>(src), hi = *reinterpret_cast<const f32x4 *>(src + 4);
                        xr[cb][s] = u32x4{pack_bf16x2(lo.x, lo.y), pack_bf16x2(lo.z, lo.w), pack_bf16x2(hi.x, hi.y), pack_bf16x2(hi.z, hi.w)};
                        *reinterpret_cast<u32x4 *>(xlp + rows2[cb] * ldxl + 32 * s + 8 * g) = xr[cb][s];
                    }
                }
            } else {
            xr[0][s] = row_a < M ? *reinterpret_cast<const u32x4 *>(x + row_a * ldx + 32 * s + 8 * g) : u32x4{0u, 0u, 0u, 0u};
            xr[1][s] = row_b < M ? *reinterpret_cast<const u32x4 *>(x + row_b * ldx + 32 * s + 8 * g) : u32x4{0u, 0u, 0u, 0u};
            }
        }
        // H / dH slots of this wave's two 16-row blocks: the block's first row is part of the SCALAR offset, rows left in the block
        // decide per lane between its (tile-independent) offset and kFfnNoRow -- selected where it is used, so that one register
        // per matrix lives through the chunk loop.  A block with no row left keeps a zero scalar offset.
        int left[2];
        unsigned hrow[2], drow[2];
        if constexpr (MODE != kFfnInfer) {
            const long long row0 = (tile * kFfnWaves + wave) * kFfnRows;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                const long long l = M - row0 - 16 * cb;
                left[cb] = __builtin_amdgcn_readfirstlane(l > 16 ? 16 : l < 0 ? 0 : (int)l);
                hrow[cb] = __builtin_amdgcn_readfirstlane(left[cb] ? (unsigned)((row0 + 16 * cb) * ldh * 2) : 0u);
                if constexpr (MODE == kFfnBwd) drow[cb] = __builtin_amdgcn_readfirstlane(left[cb] ? (unsigned)((row0 + 16 * cb) * ldd * 2) : 0u);
            }
        }
        f32x4 acc2[16][2];                                                    // out^T: tile ot, column block cb
        __syncthreads();                                                      // biases visible; previous tile's last chunk consumed
#pragma unroll
        for (int ot = 0; ot < 16; ++ot) {
            f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
            if constexpr (MODE != kFfnBwd) b4 = *reinterpret_cast<const f32x4 *>(b2l + 32 * (ot >> 1) + 8 * g + 4 * (ot & 1));
            acc2[ot][0] = b4;
            acc2[ot][1] = b4;
        }
        if (!(dbg & 1)) issue_chunk(0);
        for (int c = 0; c < nchunks; ++c) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // this wave's fragments of chunk c have landed
            if (!(dbg & 2)) __syncthreads();                                  // ... everyone's; and chunk c - 1 is consumed
            const u32x4 *w1l = reinterpret_cast<const u32x4 *>(ffn_lds + (c & 1) * kFfnBufBytes);
            const u32x4 *w2l = reinterpret_cast<const u32x4 *>(ffn_lds + (c & 1) * kFfnBufBytes + kFfnW1Bytes);
            // The chunk is ONE stream of 64 A fragments (32 of W1, 32 of W2), each feeding two MFMAs (the wave's two 16-row blocks),
            // read through a ring of three registers, two fragments AHEAD of their use: left to itself the compiler issued every
            // ds_read_b128 right before its MFMAs and waited lgkmcnt(0) -- the LDS latency once per pair of MFMAs, the matrix pipe
            // 56 % busy.  The scheduling barriers pin the order; the counted waits follow from it.  The hidden bias is added when a
            // pair is packed (accumulators start from the inline constant 0: no initialising moves).
            // Inference (kFfnSpread): four blocks of 16 steps,
            //   t =  0..15  GEMM 1 of tile pair 0   (k-step t >> 1, tile t & 1)       -> acc1a
            //   t = 16..31  GEMM 1 of tile pair 1   (k-step (t & 15) >> 1, tile 2 + (t & 1))  -> acc1b;  behind them h0 = act(acc1a)
            //   t = 32..47  GEMM 2 of pair 0        (out tile t & 15; B = h0);                           behind them h1 = act(acc1b)
            //   t = 48..63  GEMM 2 of pair 1        (out tile t & 15; B = h1)
            // so each activation has 16 steps to hide in and is cut into slices of two VALU instructions, one slice per step: an
            // even step adds the bias to the two values of one packed register, the odd step after it rounds and clamps them
            // (act_slice below).  The register packed last (step 31 / 47) belongs to column block 1: the SECOND MFMA of the next
            // step is the first to read it.
            // The 8 LDS-DMA pieces of chunk c + 1 go out one at a time, after the steps kFfnDmaFirst + i kFfnDmaEvery.
            // Every accumulator takes the operands it took in the training order below, in the same order: the same bits.
            // Training (and the development library): per k-step GEMM 1 of pair 1 and GEMM 2 of pair 0 alternate,
            //   t =  0..15  GEMM 1 of tile pair 0                      (k-step t >> 1, tile t & 1)          -> acc1a
            //   t = 16..47  per k-step s: GEMM 1 of pair 1 (2 fragments -> acc1b), GEMM 2 of pair 0 (out tiles 2s, 2s + 1; B = h0)
            //   t = 48..63  GEMM 2 of pair 1 (out tile t - 48; B = h1)
            // h0 / h1 are packed whole, two steps after their last MFMA was issued (the H / dH traffic of the training kernels is
            // part of that step), and the weight stream is issued whole after step 3.
            constexpr bool SPREAD = kFfnSpread && MODE == kFfnInfer;
            auto frag = [&](int t) -> u32x4 {
                if constexpr (SPREAD) {
                    if (t < 32) return w1l[(((t >> 4) * 2 + (t & 1)) * 8 + ((t & 15) >> 1)) * 64 + lane];
                    return w2l[((t & 15) * 2 + ((t - 32) >> 4)) * 64 + lane];
                }
                if (t < 16) return w1l[((t & 1) * 8 + (t >> 1)) * 64 + lane];
                if (t < 48) {
                    const int s = (t - 16) >> 2, r = (t - 16) & 3;
                    return r < 2 ? w1l[((2 + r) * 8 + s) * 64 + lane] : w2l[((2 * s + (r - 2)) * 2) * 64 + lane];
                }
                return w2l[((t - 48) * 2 + 1) * 64 + lane];
            };
            f32x4 acc1a[2][2], acc1b[2][2];
            u32x4 h0[2], h1[2];
            auto mm = [&](const u32x4 &a, const u32x4 &bq, const f32x4 &cacc) {
                return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(ffn_bf16x8, a), __builtin_bit_cast(ffn_bf16x8, bq), cacc, 0, 0, 0);
            };
            u32x4 hs0[2], hs1[2];                                                 // backward: the saved H of tile pair 0 / 1
            auto load_h = [&](int u, u32x4 (&hs)[2]) __attribute__((always_inline)) {
                const unsigned so = (unsigned)(c * kFfnHC + 32 * u) * 2u;
                hs[0] = __builtin_amdgcn_raw_buffer_load_b128(hrs, slot(ldh2, left[0]), hrow[0] + so, 0);
                hs[1] = __builtin_amdgcn_raw_buffer_load_b128(hrs, slot(ldh2, left[1]), hrow[1] + so, 0);
            };
            auto activate = [&](int u, const f32x4 (&acc1)[2][2], u32x4 (&h)[2], const u32x4 (&hs)[2]) {
                // + bias, round to bf16, relu: B operand of GEMM 2 (backward: round, zero where H <= 0)
                const unsigned so = (unsigned)(c * kFfnHC + 32 * u) * 2u;
                if constexpr (MODE == kFfnBwd) {
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb) {
                        h[cb].x = pack_bf16x2(acc1[0][cb].x, acc1[0][cb].y) & positive_bf16x2(hs[cb].x);
                        h[cb].y = pack_bf16x2(acc1[0][cb].z, acc1[0][cb].w) & positive_bf16x2(hs[cb].y);
                        h[cb].z = pack_bf16x2(acc1[1][cb].x, acc1[1][cb].y) & positive_bf16x2(hs[cb].z);
                        h[cb].w = pack_bf16x2(acc1[1][cb].z, acc1[1][cb].w) & positive_bf16x2(hs[cb].w);
                        __builtin_amdgcn_raw_buffer_store_b128(h[cb], drs, slot(ldd2, left[cb]), drow[cb] + so, 0);
                    }
                    return;
                }
                if (dbg & 16) {
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb) {
                        h[cb].x = pack_bf16x2(acc1[0][cb].x, acc1[0][cb].y);
                        h[cb].y = pack_bf16x2(acc1[0][cb].z, acc1[0][cb].w);
                        h[cb].z = pack_bf16x2(acc1[1][cb].x, acc1[1][cb].y);
                        h[cb].w = pack_bf16x2(acc1[1][cb].z, acc1[1][cb].w);
                    }
                    return;
                }
                const f32x4 blo = *reinterpret_cast<const f32x4 *>(b1l + c * kFfnHC + 32 * u + 8 * g);
                const f32x4 bhi = *reinterpret_cast<const f32x4 *>(b1l + c * kFfnHC + 32 * u + 8 * g + 4);
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    const f32x4 lo = acc1[0][cb] + blo, hi = acc1[1][cb] + bhi;
                    h[cb].x = relu_bf16x2(pack_bf16x2(lo.x, lo.y));          // round, then relu on the packed pair: 2 instructions
                    h[cb].y = relu_bf16x2(pack_bf16x2(lo.z, lo.w));
                    h[cb].z = relu_bf16x2(pack_bf16x2(hi.x, hi.y));
                    h[cb].w = relu_bf16x2(pack_bf16x2(hi.z, hi.w));
                    if constexpr (MODE == kFfnTrain) __builtin_amdgcn_raw_buffer_store_b128(h[cb], hrs, slot(ldh2, left[cb]), hrow[cb] + so, 0);
                }
            };
            const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
            // SPREAD: the slices of the two activations.  Pair u has 8 packed registers; register k is h[k >> 2][k & 3], made of
            // the values 2 (k & 1), + 1 of acc1[(k & 3) >> 1][k >> 2] and the biases 2 (k & 3), + 1 of the lane's 8.  Its three parts
            // run at the steps 15 + 16 u + 2 k (bias pair LDS -> registers), + 1 (two adds), + 2 (one convert, one max): every odd
            // step from 15 to 45 reads a pair, every odd step from 17 to 47 packs the register of the step before, and at a
            // scheduling barrier two values are in flight, not the pair's 8 biases (the loop has no registers for them).  The
            // arithmetic of activate() above, one register at a time: the same operations on the same values
            [[maybe_unused]] f32x2 act_bias;
            [[maybe_unused]] float act_a, act_b;
            [[maybe_unused]] auto act_slice = [&](int t) __attribute__((always_inline)) {
                if (t < 15 || t > 47) return;
                const bool odd = t & 1;
                if (odd && t < 47) {
                    const int u = (t - 15) >> 4, k = ((t - 15) & 15) >> 1, j = k & 3;
                    act_bias = *reinterpret_cast<const f32x2 *>(b1l + c * kFfnHC + 32 * u + 8 * g + 2 * j);
                }
                if (odd && t > 15) {
                    const int u = (t - 17) >> 4, k = ((t - 17) & 15) >> 1, cb = k >> 2, j = k & 3;
                    u32x4(&h)[2] = u ? h1 : h0;
                    h[cb][j] = relu_bf16x2(ffn_pack_bf16x2(act_a, act_b));    // round, then relu on the packed pair
                }
                if (!odd) {
                    const int u = (t - 16) >> 4, k = ((t - 16) & 15) >> 1, cb = k >> 2, j = k & 3, i = 2 * (j & 1);
                    const f32x4(&acc1)[2][2] = u ? acc1b : acc1a;
                    act_a = acc1[j >> 1][cb][i] + act_bias.x;
                    asm volatile("" : "+v"(act_a));                           // two v_add_f32: left alone the pair becomes one
                    act_b = acc1[j >> 1][cb][i + 1] + act_bias.y;             // v_pk_add_f32, 3.4 us slower per launch beside MFMAs
                }
            };
            auto apply = [&](int t, const u32x4 &a) {
                if constexpr (SPREAD) {
                    if (t < 32) {
                        const int s = (t & 15) >> 1, e = t & 1;
                        f32x4(&acc1)[2][2] = t < 16 ? acc1a : acc1b;
                        acc1[e][0] = mm(a, xr[0][s], s ? acc1[e][0] : zero4);
                        acc1[e][1] = mm(a, xr[1][s], s ? acc1[e][1] : zero4);
                    } else {
                        const int ot = t & 15;
                        const u32x4(&h)[2] = t < 48 ? h0 : h1;
                        acc2[ot][0] = mm(a, h[0], acc2[ot][0]);
                        acc2[ot][1] = mm(a, h[1], acc2[ot][1]);
                    }
                    act_slice(t);
                    return;
                }
                if (t < 16) {
                    const int s = t >> 1, e = t & 1;
                    acc1a[e][0] = mm(a, xr[0][s], s ? acc1a[e][0] : zero4);
                    acc1a[e][1] = mm(a, xr[1][s], s ? acc1a[e][1] : zero4);
                } else if (t < 48) {
                    const int s = (t - 16) >> 2, r = (t - 16) & 3;
                    if (r < 2) {
                        acc1b[r][0] = mm(a, xr[0][s], s ? acc1b[r][0] : zero4);
                        acc1b[r][1] = mm(a, xr[1][s], s ? acc1b[r][1] : zero4);
                    } else {
                        const int ot = 2 * s + (r - 2);
                        acc2[ot][0] = mm(a, h0[0], acc2[ot][0]);
                        acc2[ot][1] = mm(a, h0[1], acc2[ot][1]);
                    }
                } else {
                    const int ot = t - 48;
                    acc2[ot][0] = mm(a, h1[0], acc2[ot][0]);
                    acc2[ot][1] = mm(a, h1[1], acc2[ot][1]);
                }
                if (t == 17) activate(0, acc1a, h0, hs0);                     // first needed at t = 18
                if (t == 47) activate(1, acc1b, h1, hs1);                     // acc1b complete since t = 45; first needed at t = 48
                if (MODE == kFfnBwd && t == 18) load_h(1, hs1);               // acc1a's registers are free: 29 steps ahead of its use
            };
            if (!(dbg & 12)) {
                u32x4 ring[3];
                if constexpr (MODE == kFfnBwd) load_h(0, hs0);                // 17 steps of MFMAs ahead of its use
                ring[0] = frag(0);
                ring[1] = frag(1);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    ring[(t + 2) % 3] = frag(t + 2);
                    __builtin_amdgcn_sched_barrier(0);
                    apply(t, ring[t % 3]);
                    __builtin_amdgcn_sched_barrier(0);
                }
                // the weight stream of chunk c + 1, behind the first MFMAs (the pipe starts at once) and after the chunk-top barrier
                // (its buffer is free).  SPREAD: one piece after each of the steps kFfnDmaFirst + i kFfnDmaEvery, and no branch
                // around them (eight branches in the loop cost it its registers): behind the last chunk they fetch chunk 0 again,
                // into the buffer that chunk does not read -- 64 KiB of L2 traffic per tile that nobody uses, landed before the
                // vmcnt(0) below the chunk loop
                const int cnext = c + 1 < nchunks ? c + 1 : 0;
                auto dma_after = [&](int t) __attribute__((always_inline)) {
                    if constexpr (SPREAD) {
                        const int d = t - kFfnDmaFirst;
                        if (d >= 0 && d % kFfnDmaEvery == 0 && d / kFfnDmaEvery < 8) issue_piece(cnext, (c + 1) & 1, d / kFfnDmaEvery);
                    } else {
                        if (t == 3 && c + 1 < nchunks && !(dbg & 1)) issue_chunk(c + 1);
                    }
                };
                dma_after(3);
                if constexpr (SPREAD) {
#pragma unroll
                    for (int t = 4; t < 64; ++t) {
                        if (t + 2 < 64) ring[(t + 2) % 3] = frag(t + 2);
                        __builtin_amdgcn_sched_barrier(0);
                        apply(t, ring[t % 3]);
                        __builtin_amdgcn_sched_barrier(0);
                        dma_after(t);
                    }
                } else {
                    // the same steps written out at compile time: as a loop to be unrolled every iteration carries all of a step's
                    // cases, and with the training epilogues the body exceeds the unroller's size limit (the arrays then live in
                    // scratch).  So does the lumped inference loop of the development library with its timing branches.
                    ffn_static_for(std::make_integer_sequence<int, 60>{}, [&](auto tc) __attribute__((always_inline)) {
                        constexpr int t = 4 + decltype(tc)::value;
                        if (t + 2 < 64) ring[(t + 2) % 3] = frag(t + 2);
                        __builtin_amdgcn_sched_barrier(0);
                        apply(t, ring[t % 3]);
                        __builtin_amdgcn_sched_barrier(0);
                    });
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (kFfnSpread && MODE == kFfnInfer)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // the pieces issued behind the last chunk: nothing in flight
                                                                              // into LDS when the next tile, or nobody, owns it
        // the epilogue's row pointers (out, pos, out2) are derived from values the compiler cannot see before this point: hoisted
        // above the chunk loop they would occupy 12 registers there and spill the loop
        unsigned col_e = (unsigned)col;
        asm volatile("" : "+v"(col_e));
        const long long row_e = (tile * kFfnWaves + wave) * kFfnRows + col_e;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const long long row = row_e + 16 * cb;
            if constexpr (LN) {
                // out = LayerNorm(x + ffn(x)) (relation_transformer.py:272-276): the residual is the X^T fragment of k-step u
                // (x[row][32 u + 8 g ..] -- the very columns this lane holds of tile pair u); the row is spread over the 4 lanes
                // l, l ^ 16, l ^ 32, l ^ 48.  ffn(x) is rounded to bf16 first, as the unfused path stores it; fp32 two-pass statistics
                float sum = 0.f;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const u32x4 r = xr[cb][u];
                    f32x4 &lo = acc2[2 * u][cb], &hi = acc2[2 * u + 1][cb];
                    lo.x = bf16_bits_to_f32((uint16_t)f32_to_bf16_bits(lo.x)) + __builtin_bit_cast(float, r.x << 16);
                    lo.y = bf16_bits_to_f32((uint16_t)f32_to_bf16_bits(lo.y)) + __builtin_bit_cast(float, r.x & 0xffff0000u);
                    lo.z = bf16_bits_to_f32((uint16_t)f32_to_bf16_bits(lo.z)) + __builtin_bit_cast(float, r.y << 16);
                    lo.w = bf16_bits_to_f32((uint16_t)f32_to_bf16_bits(lo.w)) + __builtin_bit_cast(float, r.y & 0xffff0000u);
                    hi.x = bf16_bits_to_f32((uint16_t)f32_to_bf16_bits(hi.x)) + __builtin_bit_cast(float, r.z << 16);
                    hi.y = bf16_bits_to_f32((uint16_t)f32_to_bf16_bits(hi.y)) + __builtin_bit_cast(float, r.z & 0xffff0000u);
                    hi.z = bf16_bits_to_f32((uint16_t)f32_to_bf16_bits(hi.z)) + __builtin_bit_cast(float, r.w << 16);
                    hi.w = bf16_bits_to_f32((uint16_t)f32_to_bf16_bits(hi.w)) + __builtin_bit_cast(float, r.w & 0xffff0000u);
                    sum += ((lo.x + lo.y) + (lo.z + lo.w)) + ((hi.x + hi.y) + (hi.z + hi.w));
                }
                sum += __shfl_xor(sum, 16, 64);
                sum += __shfl_xor(sum, 32, 64);
                const float mean = sum * (1.0f / kFfnK);
                float sq = 0.f;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    f32x4 &lo = acc2[2 * u][cb], &hi = acc2[2 * u + 1][cb];
                    lo.x -= mean; lo.y -= mean; lo.z -= mean; lo.w -= mean;
                    hi.x -= mean; hi.y -= mean; hi.z -= mean; hi.w -= mean;
                    sq += ((lo.x * lo.x + lo.y * lo.y) + (lo.z * lo.z + lo.w * lo.w)) + ((hi.x * hi.x + hi.y * hi.y) + (hi.z * hi.z + hi.w * hi.w));
                }
                sq += __shfl_xor(sq, 16, 64);
                sq += __shfl_xor(sq, 32, 64);
                const float rstd = 1.0f / sqrtf(sq * (1.0f / kFfnK) + eps);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    f32x4 &lo = acc2[2 * u][cb], &hi = acc2[2 * u + 1][cb];
                    const f32x4 g0 = *reinterpret_cast<const f32x4 *>(gml + 32 * u + 8 * g), g1 = *reinterpret_cast<const f32x4 *>(gml + 32 * u + 8 * g + 4);
                    const f32x4 c0 = *reinterpret_cast<const f32x4 *>(btl + 32 * u + 8 * g), c1 = *reinterpret_cast<const f32x4 *>(btl + 32 * u + 8 * g + 4);
                    lo.x = lo.x * rstd * g0.x + c0.x; lo.y = lo.y * rstd * g0.y + c0.y; lo.z = lo.z * rstd * g0.z + c0.z; lo.w = lo.w * rstd * g0.w + c0.w;
                    hi.x = hi.x * rstd * g1.x + c1.x; hi.y = hi.y * rstd * g1.y + c1.y; hi.z = hi.z * rstd * g1.z + c1.z; hi.w = hi.w * rstd * g1.w + c1.w;
                }
            }
            if constexpr (DXF32) {
                if (row < M) {
                    float *o = outf + row * ldo + 8 * g;
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        *reinterpret_cast<f32x4 *>(o + 32 * u) = acc2[2 * u][cb];
                        *reinterpret_cast<f32x4 *>(o + 32 * u + 4) = acc2[2 * u + 1][cb];
                    }
                }
            } else if (row < M) {
                uint16_t *o = out + row * ldo + 8 * g;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const f32x4 lo = acc2[2 * u][cb], hi = acc2[2 * u + 1][cb];
                    u32x4 pk;
                    pk.x = pack_bf16x2(lo.x, lo.y);
                    pk.y = pack_bf16x2(lo.z, lo.w);
                    pk.z = pack_bf16x2(hi.x, hi.y);
                    pk.w = pack_bf16x2(hi.z, hi.w);
                    *reinterpret_cast<u32x4 *>(o + 32 * u) = pk;
                    if (LN && out2) {            // out2 = out + pos from the STORED values: the next layer's query + query_pos
                        const u32x4 pv = *reinterpret_cast<const u32x4 *>(pos + row * ldp + 8 * g + 32 * u);
                        u32x4 q;
                        q.x = f32_to_bf16_bits(__builtin_bit_cast(float, pk.x << 16) + __builtin_bit_cast(float, pv.x << 16)) |
                              (f32_to_bf16_bits(__builtin_bit_cast(float, pk.x & 0xffff0000u) + __builtin_bit_cast(float, pv.x & 0xffff0000u)) << 16);
                        q.y = f32_to_bf16_bits(__builtin_bit_cast(float, pk.y << 16) + __builtin_bit_cast(float, pv.y << 16)) |
                              (f32_to_bf16_bits(__builtin_bit_cast(float, pk.y & 0xffff0000u) + __builtin_bit_cast(float, pv.y & 0xffff0000u)) << 16);
                        q.z = f32_to_bf16_bits(__builtin_bit_cast(float, pk.z << 16) + __builtin_bit_cast(float, pv.z << 16)) |
                              (f32_to_bf16_bits(__builtin_bit_cast(float, pk.z & 0xffff0000u) + __builtin_bit_cast(float, pv.z & 0xffff0000u)) << 16);
                        q.w = f32_to_bf16_bits(__builtin_bit_cast(float, pk.w << 16) + __builtin_bit_cast(float, pv.w << 16)) |
                              (f32_to_bf16_bits(__builtin_bit_cast(float, pk.w & 0xffff0000u) + __builtin_bit_cast(float, pv.w & 0xffff0000u)) << 16);
                        *reinterpret_cast<u32x4 *>(out2 + row * ldo2 + 8 * g + 32 * u) = q;
                    }
                }
            }
        }
    }
