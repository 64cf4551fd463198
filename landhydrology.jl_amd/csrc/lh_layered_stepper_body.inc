// lh_layered_stepper_body.inc -- the body of layered_column_stepper_wave_kernel and layered_column_stepper_bound_kernel
// (lh_layered_stepper.hpp includes it once in each; DESIGN.md sections 4.22 and 4.23).  Program text, not a
// function: called through an inlined function the by-value kernel does not keep the device code it had.
// In scope where it is included: the kernels' parameters P0, L, Y, AUX, nsteps, bcv; `dt`, the step; `BOUND`, a
// constant expression; `courant`, the Courant factor of the BOUND epilogue.
    __shared__ double s_tab[M::uses_tables ? MATH_TAB_DOUBLES : 2];
    __shared__ ColC<FT> s_cls[LH_LAYERED_MAX_CLASSES];
    extern __shared__ __align__(16) unsigned char s_dyn[];
    const int n = P0.nlev; // <= 64 CW (the launcher's choice of CW)
    const int slot = int(threadIdx.x) >> 6; // column of this workgroup
    const int l = int(threadIdx.x) & 63;    // lane = CW adjacent cells
    const int cpb = int(blockDim.x) >> 6;
    // per column: (true K, -psi) of every lane's top cell and the flux of the face below its bottom cell
    FT* sK = reinterpret_cast<FT*>(s_dyn) + size_t(slot) * (LS_EXCHANGE_ARRAYS * 64);
    FT* sh = sK + 64;
    FT* sFw = sh + 64;
    const M mm(stage_math_tables<M>(P0.math_tab, s_tab));
    stage_class_table<FT, M, !NOICE>(mm, L, s_cls); // (ends on a workgroup barrier)
    DevParams<FT> P = P0; // boundary values change per stage
    const unsigned blk = xcd_block(P.xcd_remap);
    const int64_t col_raw = int64_t(blk) * cpb + slot;
    const bool have = col_raw < P.ncols;
    const int64_t col = have ? col_raw : P.ncols - 1; // spare slots shadow the last column
    constexpr bool vgf = VGF && M::uses_tables;
    const bool need_Taux = FACTORS && P.viscosity_kind;
    // planes are column-fastest, lanes here level-fastest: through LDS tiles [cpb][n] (column_stepper_kernel)
    FT* tiles = reinterpret_cast<FT*>(s_dyn);
    const int64_t col_first = int64_t(blk) * cpb;
    const int tile_n = n * cpb;
    auto request = [&](const FT* plane, int k) {
        for (int e = threadIdx.x; e < tile_n; e += blockDim.x) {
            const int lev = e / cpb, cs = e - lev * cpb;
            if (col_first + cs < P.ncols) tiles[k * tile_n + cs * n + lev] = plane[int64_t(lev) * P.stride + col_first + cs];
        }
    };
    constexpr int TILE_TI = 1, TILE_TA = NOICE ? 1 : 2;
    request(Y.v[0], 0);
    if (!NOICE) request(Y.v[1], TILE_TI);
    if (need_Taux) request(AUX.v[3], TILE_TA);
    __syncthreads();
    FT y_vl[CW], ti[CW], Ta[CW];
    unsigned kc[CW]; // the class of the lane's cells: constants of the call
    bool act[CW];    // the cell exists (and the column does)
#pragma unroll
    for (int q = 0; q < CW; ++q) {
        const int i = CW * l + q;
        const int ic = i < n ? i : n - 1;
        act[q] = i < n && have;
        y_vl[q] = have ? tiles[slot * n + ic] : FT(0);
        ti[q] = NOICE ? FT(0) : (have ? tiles[TILE_TI * tile_n + slot * n + ic] : FT(0)); // NOICE: the plane is known to be all zeros
        Ta[q] = need_Taux ? (have ? tiles[TILE_TA * tile_n + slot * n + ic] : FT(288)) : FT(288);
        // one byte per cell per call, read where it lies (the column fastest: a lane's bytes are `stride` apart)
        kc[q] = unsigned(L.cls[int64_t(ic) * P.stride + col]) & unsigned(LH_LAYERED_MAX_CLASSES - 1);
    }
    __syncthreads(); // the tiles overlay other columns' exchange arrays
    const int lt = (n - 1) / CW, qt = (n - 1) - lt * CW; // lane and slot of the top cell
    const bool at_bottom = (l == 0), at_top = (l == lt);
    // the class of the boundary cell this lane owns (the bottom lane: cell 0; the top cell's slot qt is uniform)
    unsigned kb = kc[0];
    if (!at_bottom) {
#pragma unroll
        for (int q = 1; q < CW; ++q)
            if (q == qt) kb = kc[q];
    }
    unsigned kt = kc[0]; // (a column of <= CW cells: the bottom lane owns the top cell as well)
#pragma unroll
    for (int q = 1; q < CW; ++q)
        if (q == qt) kt = kc[q];
    FT nf_acc = FT(0);
    for (int64_t s = 0; s < nsteps; ++s) {
        FT u_vl[CW]; // the stage state
#pragma unroll
        for (int q = 0; q < CW; ++q) u_vl[q] = y_vl[q];
#pragma unroll 1
        for (int stage = 0; stage < 3; ++stage) {
            if (bcv) set_stage_boundary_values(P, bcv + (s * 3 + stage) * 4);
            FT K[CW], psi[CW]; // the TRUE conductivity and -psi (see head_difference)
#pragma unroll
            for (int q = 0; q < CW; ++q) {
                const ColC<FT>& c = s_cls[kc[q]];
                FT Kr = FT(0);
                psi[q] = FT(0);
                water_closures<FT, M, FACTORS, true, false, NOICE, true, false, true>(mm, P, c, u_vl[q], ti[q], Ta[q], Kr, psi[q],
                                                                                      nullptr, vgf);
                K[q] = Kr * c.Ksat; // the two cells of a face may differ in Ksat
            }
            // the lane's top cell, for the lane above
            sK[l] = K[CW - 1];
            sh[l] = psi[CW - 1];
            wave_sync();
            // boundary faces: the lane with the bottom cell and the lane with the top cell go through
            // boundary_fluxes TOGETHER (one divergent pass, not two, when both faces need closures)
            FT Fw_b = FT(0), Fw_t = FT(0);
            if (at_bottom || at_top) {
                FT bv = u_vl[0], bti = ti[0], bT = Ta[0], bK = K[0], bpsi = psi[0];
                if (!at_bottom) {
#pragma unroll
                    for (int q = 1; q < CW; ++q)
                        if (q == qt) { bv = u_vl[q]; bti = ti[q]; bT = Ta[q]; bK = K[q]; bpsi = psi[q]; }
                }
                FT fe, fw;
                boundary_fluxes<FT, M, MODEL_RICHARDS, FACTORS, NOICE>(mm, P, s_cls[kb], at_bottom ? FACE_BOTTOM : FACE_TOP, col, bv,
                                                                       bti, bT, bK, -bpsi, fe, fw, nullptr, nullptr, vgf);
                fw = fw * P.inv_dz;
                if (at_bottom) Fw_b = fw;
                else Fw_t = fw;
                if (at_bottom && at_top) { // a column of <= CW cells: the same lane owns both faces
#pragma unroll
                    for (int q = 0; q < CW; ++q)
                        if (q == qt) { bv = u_vl[q]; bti = ti[q]; bT = Ta[q]; bK = K[q]; bpsi = psi[q]; }
                    boundary_fluxes<FT, M, MODEL_RICHARDS, FACTORS, NOICE>(mm, P, s_cls[kt], FACE_TOP, col, bv, bti, bT, bK, -bpsi, fe,
                                                                           Fw_t, nullptr, nullptr, vgf);
                    Fw_t = Fw_t * P.inv_dz;
                }
            }
            // F[q]: the face below the lane's cell q; F[CW]: the face above its top cell.  Every interior face once,
            // lower cell first, with layered_rhs_kernel's line.
            FT Fw[CW + 1];
#pragma unroll
            for (int q = 0; q <= CW; ++q) Fw[q] = FT(0);
            if (at_bottom) Fw[0] = Fw_b;
            else Fw[0] = -(sK[l - 1] + K[0]) * (head_difference(psi[0], sh[l - 1], P.dz) * P.cg2);
#pragma unroll
            for (int q = 1; q < CW; ++q) Fw[q] = -(K[q - 1] + K[q]) * (head_difference(psi[q], psi[q - 1], P.dz) * P.cg2);
            // the face above the lane's top cell is the face below the next lane's bottom cell
            sFw[l] = Fw[0];
            wave_sync();
            if (l < 63) Fw[CW] = sFw[l + 1];
            if (at_top) { // the face above the column's top cell (slot qt) is the boundary
#pragma unroll
                for (int q = 0; q < CW; ++q)
                    if (q == qt) Fw[q + 1] = Fw_t;
            }
#pragma unroll
            for (int q = 0; q < CW; ++q) {
                const FT dvl = Fw[q] - Fw[q + 1];
                if (act[q]) nf_acc = fma_ft(dvl, FT(0), nf_acc);
                u_vl[q] = ssprk33_stage_value<FT>(stage, y_vl[q], u_vl[q], dvl, dt);
            }
            wave_sync(); // the neighbours have read this stage's LDS values
        }
#pragma unroll
        for (int q = 0; q < CW; ++q) y_vl[q] = u_vl[q];
    }
    if constexpr (BOUND) {
        // The scalar stepper's BOUND epilogue (lh_kernels_impl.hpp) with every column constant taken per cell: one
        // more closure pass over the final state with the slope, the TRUE conductivity as the time loop forms it
        // (no per-column Ksat at the end), and every cell's slope divided by its OWN class's n m before any maximum
        // -- the two cells of a face may differ in n.  No heat term.
        // (every neighbour has read the last stage's LDS values: the wave_sync that ends a stage)
        FT K[CW];
        float dpsi[CW];
        // A NaN vartheta_l takes the closures' saturated branch (K = Ksat and the slope 1 / S_s, as the reference's
        // `S < 1 ? ... : 1` does): finite coefficients from no state at all.  Such a column has no bound and is left
        // out like one whose maximum is NaN; the time loop flags it.
        bool no_state = false;
#pragma unroll
        for (int q = 0; q < CW; ++q) {
            no_state = no_state || (act[q] && y_vl[q] != y_vl[q]);
            const ColC<FT>& c = s_cls[kc[q]];
            FT Kr = FT(0), npsi = FT(0); // (-psi: not needed by the bound)
            float nm_dpsi = 0.0f;        // n m d psi / d vl, kept finite (slope32)
            water_closures<FT, M, FACTORS, true, true, NOICE, true, false, true>(mm, P, c, y_vl[q], ti[q], Ta[q], Kr, npsi, &nm_dpsi, vgf);
            K[q] = Kr * c.Ksat;
            // n < 2: the factor exceeds 1 and a saturated slope would leave the Float32 range again, while the K of
            // such a bone-dry clay-like cell underflows to 0 -- 0 x Inf must not poison the column's maximum
            dpsi[q] = finite_nonneg(nm_dpsi * float(FT(1) / (c.n * c.m)));
        }
        // the lane's top cell, for the lane above (a float passes through an FT word unchanged)
        sK[l] = K[CW - 1];
        sh[l] = FT(dpsi[CW - 1]);
        wave_sync();
        float Dmax = no_state ? __builtin_nanf("") : 0.0f; // twice the largest diffusivity of the column (a NaN wins every maximum)
#pragma unroll
        for (int q = 0; q < CW; ++q) { // the interior face below cell q
            const int i = CW * l + q;
            if (i > 0 && i < n) {
                FT K_p;
                float dpsi_p;
                if (q > 0) { // the cell below is the lane's own (q is a constant of the unrolled loop)
                    K_p = K[q - 1];
                    dpsi_p = dpsi[q - 1];
                } else {
                    K_p = sK[l - 1];
                    dpsi_p = float(sh[l - 1]);
                }
                Dmax = max_nonneg(Dmax, float(K_p + K[q]) * max_nonneg(dpsi_p, dpsi[q]));
            }
        }
        // the boundary cells' own coefficients; Dirichlet faces: half a cell away, the coefficients of the face state
        // in the boundary cell's own class (face_state leaves K_f = 0 on any other kind of face)
        auto boundary_terms = [&](int face, int q_cell, unsigned k_cell) {
            FT bv = y_vl[0], bti = ti[0], bT = Ta[0], bK = K[0];
            float bdpsi = dpsi[0];
#pragma unroll
            for (int q = 1; q < CW; ++q)
                if (q == q_cell) { bv = y_vl[q]; bti = ti[q]; bT = Ta[q]; bK = K[q]; bdpsi = dpsi[q]; }
            const FT K_f = face_state<FT, M, MODEL_RICHARDS, FACTORS, NOICE>(mm, P, s_cls[k_cell], face, col, bv, bti, bT, vgf).K;
            Dmax = max_nonneg(Dmax, 2.0f * float(bK) * bdpsi);
            Dmax = max_nonneg(Dmax, 4.0f * float(fmax_ft(K_f, K_f > FT(0) ? bK : FT(0))) * bdpsi);
        };
        if (at_bottom || at_top) boundary_terms(at_bottom ? FACE_BOTTOM : FACE_TOP, at_bottom ? 0 : qt, kb);
        if (at_bottom && at_top) boundary_terms(FACE_TOP, qt, kt); // a column of <= CW cells
        // the wave's maximum (every lane of the wave is here: the kernel has no early exit)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) Dmax = max_nonneg(Dmax, __shfl_xor(Dmax, off, 64));
        if (l == 0 && have) { // (a column whose maximum is NaN is dropped; its status bit comes from the time loop)
            const float dmax = Dmax == Dmax ? max_nonneg(0.0f, Dmax) : 0.0f;
            if (dmax > 0.0f) bound_publish<FT>(P, courant, dmax);
        }
    }
    if (!BOUND || nsteps > 0) { // (uniform: a zero-step BOUND launch is the bound of Y and writes no plane)
        __syncthreads(); // the tiles overlay other columns' exchange arrays
#pragma unroll
        for (int q = 0; q < CW; ++q) {
            const int i = CW * l + q;
            if (i < n) tiles[slot * n + i] = y_vl[q];
        }
        __syncthreads();
        for (int e = threadIdx.x; e < tile_n; e += blockDim.x) {
            const int lev = e / cpb, cs = e - lev * cpb;
            if (col_first + cs < P.ncols) Y.v[0][int64_t(lev) * P.stride + col_first + cs] = tiles[cs * n + lev];
        }
    }
    if (have && nf_acc != nf_acc) atomicOr(P.status, 1u);
