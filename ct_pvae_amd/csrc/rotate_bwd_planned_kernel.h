// rotate_bwd_planned_kernel.h -- the TEXT of the planned backward kernel (described in rotate_plan.hip, which includes this file once
// per store policy of the gradient image): CTPVAE_BWD_PLANNED_KERNEL is the kernel's name, CTPVAE_BWD_PLANNED_STORE its StorePolicy
// (common.h).  Not a header of its own: it uses rotate_plan.hip's helpers.  One text, so that the forms differ in their store
// instructions alone; a second NAME rather than a template parameter, so that the plain kernels keep the names the profiles and the
// ISA tests know them by -- and, compiled from the same tokens, their instructions.
template <int PPT, int MAXT, int NS, int DUP = 1, bool SHORT = false>
__global__ __launch_bounds__(MAXT) void CTPVAE_BWD_PLANNED_KERNEL(const float *__restrict__ gsino, PlanGeom g, BwdLayout L,
                                                                 const uint4 *__restrict__ idx, int tiles_y, int g_S,
                                                                 SliceScale scale, float *__restrict__ gimg, unsigned inv_tiles,
                                                                 unsigned inv_nxb, unsigned stage_magic, unsigned idx_req)
{
    static_assert(!SHORT || DUP == 1, "SHORT launches are tf_compat plans of at most 32 angles");
    typedef typename SliceVec<NS>::type vec_t;
    constexpr int kChunk = kBwdChunk / NS;
    extern __shared__ float lds[];
    const int lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    const int wave = SHORT ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : threadIdx.x >> 6;
    const int tiles = L.nXB * tiles_y;
    const int units = (g_S + NS - 1) / NS;
    // Workgroups b and b + 8 share an XCD (round-robin dispatch; speed only): the tiles of one slice (pair) are placed
    // on one XCD so that its cotangent rows are fetched into one L2 -- block = (u / 8) * 8 * tiles + tile * 8 + u % 8.
    int u, tile;
    if constexpr (SHORT) {
        const unsigned per8 = 8u * tiles, octet = div_by_magic_floor(blockIdx.x >> 3, inv_tiles, tiles), rem = blockIdx.x - octet * per8;
        if ((int)(octet + 1) * 8 <= units) {
            tile = rem >> 3;
            u = octet * 8 + (rem & 7);
        } else {
            const unsigned ru = div_by_magic_floor(rem, inv_tiles, tiles);
            u = octet * 8 + ru;
            tile = rem - ru * tiles;
        }
    } else {
        // (divisions by multiplication, div_magic: inv_tiles == 0 -- the host's "operands too large" -- divides)
        const int per8 = 8 * tiles;
        const int octet = inv_tiles ? (int)div_by_magic(blockIdx.x >> 3, inv_tiles) : (int)blockIdx.x / per8, rem = blockIdx.x - octet * per8;
        if ((octet + 1) * 8 <= units) {
            tile = rem >> 3;
            u = octet * 8 + (rem & 7);
        } else {   // the last, partial octet is laid out unit-major
            const int ru = inv_tiles ? (int)div_by_magic((unsigned)rem, inv_tiles) : rem / tiles;
            u = octet * 8 + ru;
            tile = rem - ru * tiles;
        }
    }
    const int s = u * NS;
    const bool has2 = NS == 2 && s + 1 < g_S;   // an odd batch ends with a half-empty pair (slice s staged twice)
    CTPVAE_PSTAMP(0);
    // (the per-slice factors are wanted at the very end: a SHORT launch asks for them behind its barrier)
    float k0 = 1.0f, k1 = 1.0f;
    if constexpr (!SHORT) k0 = scale.at(s), k1 = has2 ? scale.at(s + 1) : 1.0f;
    const int ty = SHORT ? (int)div_by_magic_floor((unsigned)tile, inv_nxb, (unsigned)L.nXB)
                         : (inv_tiles ? (int)div_by_magic((unsigned)tile, inv_nxb) : tile / L.nXB),
              xb = tile - ty * L.nXB;
    // (SHORT: at most 32 x 255 cotangents per slice, and a plan of two index groups: 2 H Wpad < 2^32 vectors with check_plan_geom's
    // PH PW < 2^24 -- unsigned 32-bit products)
    const size_t slice_elems = SHORT ? (size_t)(unsigned)(g.A * g.PW) : (size_t)g.A * g.PW;
    const float *gs = SHORT ? gsino + (size_t)s * slice_elems : gsino + (size_t)s * g.A * g.PW;
    const int xcol = xb * 64 + lane;
    const int y0 = ty * (nwaves * PPT) + wave;   // this wave's rows: y0, y0 + nwaves, ...
    vec_t acc[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) acc[k] = 0.0f;
    const uint4 *p = idx + (size_t)xcol;
    // Index vectors of TWO groups of sixteen angles in flight (round 4; SHORT launches hold both of theirs anyway): with one,
    // every wave of a many-angle launch waited out an L2 round trip per group -- SQ_WAIT_ANY was 46 % of the wave cycles at
    // B = 50 x 180 angles with the LDS array 22 % busy -- and all sixteen waves of the CU's one workgroup did so together.
    uint4 q[2][PPT];
    // (SHORT: the owned rows' offsets in a group, row * Wpad + column, once for every request below -- each sits in a block of its own; a
    // request's address is the plan's, a scalar, and a 32-bit byte offset: H Wpad < 2^24 with H < 2^16, Wpad <= 256, so the plan is < 2^30 bytes)
    [[maybe_unused]] unsigned erow[PPT];
    if constexpr (SHORT) {
#pragma unroll
        for (int k = 0; k < PPT; ++k) erow[k] = (unsigned)min(y0 + k * nwaves, g.H - 1) * (unsigned)L.Wpad + (unsigned)xcol;
    }
    auto load_group = [&](int a16, auto slot_tag) {
        constexpr int SLOT = decltype(slot_tag)::value;
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int y = min(y0 + k * nwaves, g.H - 1);   // rows past the slice re-read the last row, never stored
#ifdef CTPVAE_TUNE_BWD_NOIDX
            if (a16 > 0) continue;   // timing only: every group reuses the first index vectors (no index streaming)
#endif
            if constexpr (SHORT) q[SLOT][k] = *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(idx) + (((unsigned)(a16 * g.H) * (unsigned)L.Wpad + erow[k]) << 4));
            else q[SLOT][k] = p[((size_t)a16 * g.H + y) * L.Wpad];
        }
    };
    // SHORT: the launch's LAST index vector (q2nd), of which the gathers read the first 1 .. 4 dwords, comes either whole -- the uint4 of
    // the second group, which IS the first when there is one -- or from the plan's compact tail section, which holds exactly the dwords
    // that are read as records of 1 .. 3 dwords per (row, padded column) behind the uint4 array (NA16 H Wpad vectors: a multiple of
    // 1 KB): one load of that many dwords per owned row, a wave's 64 records one contiguous run (byte offsets < 12 H Wpad < 2^32); the
    // other components of q2nd are then never read.  Which requests the launch makes is a launch constant, idx_req (launch_bwd_planned
    // derives it from the same A as the gathers' cases below), one BIT per request: to the compiler five independent jumps over a short
    // block each -- from equality tests of a record size it builds a switch, which its structurizer flattens into twice the
    // instructions.  The full first vector is requested last: the compiler guards the q2nd registers of one block against the loads
    // of the blocks before it with waits, which find nothing in flight as only one of those blocks is ever run.
    [[maybe_unused]] uint4 q2nd[PPT];
    if constexpr (!SHORT) {
        load_group(0, std::integral_constant<int, 0>{});       // index loads fly while the cotangent rows land
        load_group(min(1, L.NA16 - 1), std::integral_constant<int, 1>{});
    } else {
        const char *tail = reinterpret_cast<const char *>(idx + (unsigned)(L.NA16 * g.H) * (unsigned)L.Wpad);
        if (idx_req & kIdxReqTailWhole) {
#pragma unroll
            for (int k = 0; k < PPT; ++k)   // (its second group)
                q2nd[k] = *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(idx) + (((unsigned)(min(1, L.NA16 - 1) * g.H) * (unsigned)L.Wpad + erow[k]) << 4));
            asm volatile("; whole tail vectors");
        }
        auto tail_rows = [&](auto t_tag) {
            constexpr int T = decltype(t_tag)::value;
            struct Rec { unsigned w[T]; };
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const Rec r = *reinterpret_cast<const Rec *>(tail + erow[k] * (unsigned)sizeof(Rec));
                q2nd[k].x = r.w[0];
                if constexpr (T > 1) q2nd[k].y = r.w[1];
                if constexpr (T > 2) q2nd[k].z = r.w[2];
            }
            // (a case ends in a line of its own: the compiler would otherwise share the cases' first dwords in one load behind them)
            asm volatile("; tail records of %0 dwords" ::"n"(T));
        };
        if (idx_req & kIdxReqTail1) tail_rows(std::integral_constant<int, 1>{});
        if (idx_req & kIdxReqTail2) tail_rows(std::integral_constant<int, 2>{});
        if (idx_req & kIdxReqTail3) tail_rows(std::integral_constant<int, 3>{});
        if (idx_req & kIdxReqFirst) load_group(0, std::integral_constant<int, 0>{});   // (records and A <= 12: the launch loads no uint4 at all)
    }

    const int VA = g.A * DUP;                            // virtual angles (= angles unless DUP = 2)
    const int chunk = min(L.NA16 * 16, kChunk * DUP);    // virtual angles per staged chunk (a multiple of 16)
    // Pairs in 16-wave workgroups (many angles, several chunks): the cotangent rows of chunk c + 1 are requested into
    // registers (two units per lane) before the gathers of chunk c and written to LDS after them -- each chunk's load
    // round trip hides behind the previous chunk's gather phase instead of standing between two barriers.
    constexpr bool kPipe = NS == 2 && !SHORT;       // (the single-slice form has no registers to spare: 143 VGPRs with it)
    constexpr int kAheadUnits = 2;                  // 32 rows of a pair over 16 waves
    StagedRows<NS, kPipe ? kAheadUnits : 1> ahead;
    bool ahead_valid = false;
    auto chunk_srcs = [&](int ac, const float *(&srcs)[NS]) {
        srcs[0] = gs + (size_t)ac * g.PW;
        if constexpr (NS == 2) srcs[1] = gs + (has2 ? slice_elems : 0) + (size_t)ac * g.PW;
    };
    // (SHORT: the loop is its one trip with acv = 0 -- written so that the compiler sees it)
    for (int acv = 0; acv < (SHORT ? 1 : VA); acv += (SHORT ? 1 : chunk)) {
        const int nav = SHORT ? VA : min(chunk, VA - acv);
        const int na4 = (nav + 3) & ~3;             // taps are consumed a dword (4 virtual angles) at a time
        const int ac = acv / DUP;                   // first staged (real) angle of the chunk
        const int na = (nav + DUP - 1) / DUP;       // staged rows
        const int na_z = (na4 + DUP - 1) / DUP;     // rows a tap of this chunk may name
        if (acv > 0) __syncthreads();
        // a dead tap is byte 255: only cell 255 of every row (never a bin: PW <= 255) must hold 0.0f
        auto stage_general = [&] {
            if constexpr (NS == 1) {
                stage_rows(lds, gs + (size_t)ac * g.PW, na, g.PW, g.PW, kBwdPitch, false, lane, wave, nwaves);
            } else {
                const float *srcs[NS];
                chunk_srcs(ac, srcs);
                stage_rows_interleaved<2>(lds, srcs, na, g.PW, g.PW, kBwdPitch, false, lane, wave, nwaves);
            }
        };
        if constexpr (SHORT) {   // (na_z <= 32 rows: one store of the first lanes, issued while the rows are in flight)
            auto zero_cells = [&] {
                if ((int)threadIdx.x < na_z) reinterpret_cast<vec_t *>(lds)[threadIdx.x * kBwdPitch + 255] = 0.0f;
            };
            if (stage_magic != 0) {   // launch-uniform
                const float *srcs[NS];
                chunk_srcs(0, srcs);
                stage_contig_rows<NS, 8 / NS>(lds, srcs, na, g.PW, kBwdPitch, stage_magic, threadIdx.x, blockDim.x, zero_cells);
            } else {
                zero_cells();
            }
        } else {
            for (int t = threadIdx.x; t < na_z * NS; t += blockDim.x) lds[((t / NS) * kBwdPitch + 255) * NS + (t % NS)] = 0.0f;
            if (ahead_valid) ahead.commit(lds, kBwdPitch);           // requested during the previous chunk's gathers
            else stage_general();
        }
        ahead_valid = false;
        if (kPipe && acv + chunk < VA) {            // wave-uniform
            const float *srcs[NS];
            chunk_srcs(ac + chunk / DUP, srcs);
            const int nna = (min(chunk, VA - (acv + chunk)) + DUP - 1) / DUP;
            if (StagedRows<NS, kPipe ? kAheadUnits : 1>::fits(srcs, nna, g.PW, g.PW, nwaves)) {
                ahead.issue(srcs, nna, g.PW, g.PW, lane, wave, nwaves);
                ahead_valid = true;
            }
        }
        // (the gradient image's address is asked for with the other launch constants: left to the compiler, its scalar load sinks to the
        // stores, where a CU's first workgroup waits out a cold scalar-cache miss with nothing left to hide it)
        if constexpr (SHORT) asm volatile("" ::"s"(gimg));
        if (acv == 0) CTPVAE_PSTAMP(1);
        __syncthreads();
        if constexpr (SHORT) {
            k0 = scale.at(s), k1 = has2 ? scale.at(s + 1) : 1.0f;
            // Rows that stage_contig_rows cannot take (PW % 4 != 0, an unaligned tensor) go through the general stagers, and what a
            // workgroup that is small for its rows could not request in one batch follows, BEHIND the barrier: the launches this form is
            // written for run straight into their barrier and jump over this block.
            const bool more = stage_magic != 0 && contig_rows_more<8 / NS>(na, g.PW, blockDim.x);
            if (stage_magic == 0 || more) {   // launch-uniform
                if (more) {
                    const float *srcs[NS];
                    chunk_srcs(0, srcs);
                    stage_contig_rows_rest<NS, 8 / NS>(lds, srcs, na, g.PW, kBwdPitch, stage_magic, threadIdx.x, blockDim.x);
                } else {
                    stage_general();
                }
                __syncthreads();
            }
        }
        if (acv == 0) CTPVAE_PSTAMP(2);
        if constexpr (SHORT) {
            // The launch's na4 / 4 = 1 .. 8 index dwords, each executed as what it is: T dwords of the index vectors qq (staged rows
            // AL .. AL + 4 T - 1) are 4 T unpacks, gathers and, behind them, adds per owned row -- straight-line code per T, no
            // register zeroed to stand in for a tap the launch does not have.  (The accumulators start at +0.0f and can therefore
            // never be -0.0f: an add of +0.0f that is not executed changes no bit.)
            auto taps = [&](auto al_tag, auto t_tag, const uint4(&qq)[PPT]) {
                constexpr int AL = decltype(al_tag)::value, T = decltype(t_tag)::value;
                vec_t v[PPT][4 * T];
#pragma unroll
#ifdef CTPVAE_TUNE_BWD_NOLDS
                for (int k = 0; k < PPT; ++k)   // timing only: no gathers, the index words stand in for the taps
                    for (int e = 0; e < 4 * T; ++e) v[k][e] = __uint_as_float((&qq[k].x)[e & 3] & 0x3fffffu);
#else
                for (int k = 0; k < PPT; ++k) gather_dwords<AL, T, NS>(lds, qq[k], v[k]);
#endif
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int e = 0; e < 4 * T; ++e)   // ascending angle; the rows' sums side by side: no add waits for the one before it
#pragma unroll
                    for (int k = 0; k < PPT; ++k) acc[k] += v[k][e];
                // (a case ends in a line of its own: the cases' last adds look alike, and the compiler's branch folder would otherwise
                // share them in one block behind one more jump)
                asm volatile("; rows %0 .. of %1 dwords" ::"n"(AL), "n"(T));
            };
            // the last 1 .. 4 dwords, read from the second index vectors (which ARE the first when there is one group): one
            // wave-uniform branch into the four cases
            auto tail = [&](auto al_tag) {
                const int r = na4 - decltype(al_tag)::value;   // 4, 8, 12 or 16 taps
                if (r < 8) taps(al_tag, std::integral_constant<int, 1>{}, q2nd);
                else if (r < 12) taps(al_tag, std::integral_constant<int, 2>{}, q2nd);
                else if (r < 16) taps(al_tag, std::integral_constant<int, 3>{}, q2nd);
                else taps(al_tag, std::integral_constant<int, 4>{}, q2nd);
            };
            if (na4 <= 16) {                                 // launch-uniform
                tail(std::integral_constant<int, 0>{});
            } else {
                taps(std::integral_constant<int, 0>{}, std::integral_constant<int, 4>{}, q[0]);
                tail(std::integral_constant<int, 16>{});
            }
        }
        // up to four (eight with DUP = 2) groups of sixteen virtual angles, unrolled so that every row offset is an immediate
        auto group = [&](auto al_tag) {
            constexpr int AL = decltype(al_tag)::value;
            if constexpr (!SHORT && AL < kChunk * DUP) {
                if (AL >= na4) return;                       // wave-uniform
                const int n_live = min(16, na4 - AL);
                {
                    // the chunks hold an even number of groups, so a group's slot in the two-deep index queue is a constant;
                    // taps in two halves of eight (a wave holds at most 15 LDS operations in flight anyway): the registers of
                    // the other half are what pays for the second index group
                    constexpr int SLOT = (AL / 16) & 1;
                    constexpr int ROW = kBwdPitch * 4 * NS;   // bytes per staged row
                    // one index dword = four angles at a time for all PPT rows: PPT x 4 gathers in flight, added in angle order
                    auto quarter = [&](auto d_tag) {
                        constexpr int D = decltype(d_tag)::value;
                        if (4 * D >= n_live) return;                 // wave-uniform: a partial last group skips whole dwords
                        vec_t v[PPT][4];
#pragma unroll
                        for (int k = 0; k < PPT; ++k) {
                            const unsigned w = D == 0 ? q[SLOT][k].x : D == 1 ? q[SLOT][k].y : D == 2 ? q[SLOT][k].z : q[SLOT][k].w;
#ifdef CTPVAE_TUNE_BWD_NOLDS
                            for (int e = 0; e < 4; ++e) v[k][e] = __uint_as_float(w & 0x3fffffu);
#else
                            int b0, b1, b2, b3;
                            unpack4<NS == 1 ? 2 : 3>(w, b0, b1, b2, b3);
                            v[k][0] = lds_at_vec<NS>(lds, b0 + ((AL + 4 * D + 0) / DUP) * ROW);
                            v[k][1] = lds_at_vec<NS>(lds, b1 + ((AL + 4 * D + 1) / DUP) * ROW);
                            v[k][2] = lds_at_vec<NS>(lds, b2 + ((AL + 4 * D + 2) / DUP) * ROW);
                            v[k][3] = lds_at_vec<NS>(lds, b3 + ((AL + 4 * D + 3) / DUP) * ROW);
#endif
                        }
                        if constexpr (D == 3) {   // this group's index vectors are consumed: request the group after next
                            const int next = (acv + AL) / 16 + 2;
                            if (next < L.NA16) load_group(next, std::integral_constant<int, SLOT>{});
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int k = 0; k < PPT; ++k)
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[k] += v[k][e];
                        __builtin_amdgcn_sched_barrier(0);
                    };
                    quarter(std::integral_constant<int, 0>{});
                    quarter(std::integral_constant<int, 1>{});
                    quarter(std::integral_constant<int, 2>{});
                    quarter(std::integral_constant<int, 3>{});
                    // (a partial group is the launch's last: nothing is requested behind it)
                }
            }
        };
        group(std::integral_constant<int, 0>{});
        group(std::integral_constant<int, 16>{});
        group(std::integral_constant<int, 32>{});
        group(std::integral_constant<int, 48>{});
        group(std::integral_constant<int, 64>{});
        group(std::integral_constant<int, 80>{});
        group(std::integral_constant<int, 96>{});
        group(std::integral_constant<int, 112>{});
    }
    if (xcol < g.W) {
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int y = y0 + k * nwaves;
            if (y < g.H) {
                if constexpr (NS == 1) {
                    store_f32<CTPVAE_BWD_PLANNED_STORE>(k0 * acc[k], &gimg[((size_t)s * g.H + y) * g.W + xcol]);
                } else {
                    store_f32<CTPVAE_BWD_PLANNED_STORE>(k0 * acc[k].x, &gimg[((size_t)s * g.H + y) * g.W + xcol]);
                    if (has2) store_f32<CTPVAE_BWD_PLANNED_STORE>(k1 * acc[k].y, &gimg[((size_t)(s + 1) * g.H + y) * g.W + xcol]);
                }
            }
        }
    }
    CTPVAE_PSTAMP(3);
}
