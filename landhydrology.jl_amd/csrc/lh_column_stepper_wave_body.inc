// lh_column_stepper_wave_body.inc -- the body of column_stepper_wave_kernel (lh_kernels_impl.hpp) and of
// series_column_stepper_wave_kernel (lh_series_stepper.hpp; DESIGN.md section 4.31), included once in each.
// Program text, not a function (as lh_layered_stepper_body.inc): the first kernel keeps the device code it had.
// In scope where it is included: the template parameters FT, MODEL, FACTORS, PERCOL, M, CW, NOICE, VGF and the
// constant expression BOUND; P0, Y, AUX, dt_value, dt_device, nsteps; and what the two kernels differ in --
// two macros, textual so that the first kernel's statements are the ones it had --
//   LH_CSW_FACE_VALUES_FIXED(face)   the boundary values of the face are constants of the call
//   LH_CSW_STAGE_BOUNDARY_VALUES     a statement: the values of stage `stage` of step `s` into P.bc_value (`col` is the column)
    constexpr bool WATER = (MODEL != MODEL_HEAT);
    constexpr bool HEAT = (MODEL != MODEL_RICHARDS);
    __shared__ double s_tab[M::uses_tables ? MATH_TAB_DOUBLES : 2];
    extern __shared__ __align__(16) unsigned char s_dyn[];
    const int n = P0.nlev; // <= 64 CW (the launcher's choice of CW)
    const int slot = int(threadIdx.x) >> 6; // column of this workgroup
    const int l = int(threadIdx.x) & 63;    // lane = CW adjacent cells
    const int cpb = int(blockDim.x) >> 6;
    const FT dt = dt_device ? *dt_device : dt_value;
    // per column: the top cell of every lane -- (K, -psi), (T, kappa), rho_e_l K as the model needs --
    // and the flux(es) of the face below every lane's bottom cell; 64 words each
    // (+ CS_FACE_WORDS per column: K, psi, kappa of the face state of a Dirichlet face, bottom and top)
    constexpr int NEX = cs_exchange_arrays<MODEL>();
    constexpr int NARR = NEX + cs_flux_arrays<MODEL>();
    constexpr size_t COLW = size_t(NARR) * 64 + CS_FACE_WORDS;
    const StepperLds<FT, MODEL> ex(reinterpret_cast<FT*>(s_dyn) + size_t(slot) * COLW, 64);
    FT* sFw = ex.K + size_t(NEX) * 64;
    FT* sFe = WATER ? sFw + 64 : sFw;
    FT* sFace = ex.K + size_t(NARR) * 64;
    const M mm(stage_math_tables<M>(P0.math_tab, s_tab));
    if (!M::uses_tables) __syncthreads();
    DevParams<FT> P = P0; // boundary values change per stage
    const unsigned blk = xcd_block(P.xcd_remap);
    const int64_t col_raw = int64_t(blk) * cpb + slot;
    const int64_t col = col_raw < P.ncols ? col_raw : P.ncols - 1; // spare slots shadow the last column
    ColC<FT> c = make_colc<FT, M>(P, col, PERCOL);
    if (WATER && !NOICE) finish_colc<FT, M>(mm, c);
    // one wave = one column: its per-column constants are uniform (rhs_kernel, one LANE per column,
    // has to keep them in vector registers)
    if constexpr (PERCOL) c = wave_uniform(c);
    constexpr bool vgf = VGF && M::uses_tables;
    const FT cgT = P.cg2;
    FT Ksc, cgw;
    flux_scales<FT, M>(P, c, Ksc, cgw);
    const bool need_Taux = (MODEL == MODEL_RICHARDS) && FACTORS && P.viscosity_kind;
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
    // (level-uniform prescribed fields of Ya come from their [nlev] arrays: DevParams::aux_prof)
    const FT* pf_vl = MODEL == MODEL_HEAT ? P.aux_prof[0] : nullptr;
    const FT* pf_ti = MODEL == MODEL_HEAT ? P.aux_prof[1] : nullptr;
    const FT* pf_T = need_Taux ? P.aux_prof[3] : nullptr;
    if (!pf_vl) request(MODEL == MODEL_HEAT ? AUX.v[0] : Y.v[0], 0);
    if (!NOICE && !pf_ti) request(MODEL == MODEL_HEAT ? AUX.v[1] : Y.v[1], 1);
    if (HEAT) request(Y.v[2], 2);
    if (need_Taux && !pf_T) request(AUX.v[3], 3);
    __syncthreads();
    FT y_vl[CW], y_re[CW], ti[CW], Ta[CW];
    bool act[CW]; // the cell exists (and the column does)
#pragma unroll
    for (int q = 0; q < CW; ++q) {
        const int i = CW * l + q;
        const int ic = i < n ? i : n - 1;
        act[q] = i < n && col_raw < P.ncols;
        const bool have = col_raw < P.ncols;
        y_vl[q] = pf_vl ? pf_vl[ic] : (have ? tiles[slot * n + ic] : FT(0));
        ti[q] = NOICE ? FT(0) : (pf_ti ? pf_ti[ic] : (have ? tiles[tile_n + slot * n + ic] : FT(0))); // NOICE: the theta_i plane is known to be all zeros
        y_re[q] = (HEAT && have) ? tiles[2 * tile_n + slot * n + ic] : FT(0);
        Ta[q] = need_Taux ? (pf_T ? pf_T[ic] : (have ? tiles[3 * tile_n + slot * n + ic] : FT(288))) : FT(288);
    }
    __syncthreads(); // the tiles overlay other columns' exchange arrays
    const int lt = (n - 1) / CW, qt = (n - 1) - lt * CW; // lane and slot of the top cell
    const bool at_bottom = (l == 0), at_top = (l == lt);
    // Dirichlet faces: the closures of the FACE state -- a whole extra closure pass by one lane while
    // its wave waits -- read the boundary value, the boundary cell's theta_i and (some models) its
    // vartheta_l or T.  With constant boundary values and none of those moving (face_state_is_static)
    // they are constants of the call: evaluated once here, kept in LDS, and a stage only assembles
    // the two fluxes from them (boundary_fluxes_from) -- the same numbers as boundary_fluxes.
    const bool hoist_b = LH_CSW_FACE_VALUES_FIXED(FACE_BOTTOM) && face_state_is_static<FT, MODEL, FACTORS>(P, FACE_BOTTOM);
    const bool hoist_t = LH_CSW_FACE_VALUES_FIXED(FACE_TOP) && face_state_is_static<FT, MODEL, FACTORS>(P, FACE_TOP);
    auto hoist_face = [&](int face, int q_cell) {
        FT bv = y_vl[0], bti = ti[0], bT = Ta[0];
#pragma unroll
        for (int q = 1; q < CW; ++q)
            if (q == q_cell) { bv = y_vl[q]; bti = ti[q]; bT = Ta[q]; }
        const FaceState<FT> fs = face_state<FT, M, MODEL, FACTORS, NOICE>(mm, P, c, face, col, bv, bti, bT, vgf);
        FT* dst = sFace + (face == FACE_BOTTOM ? 0 : 3);
        dst[0] = fs.K;
        dst[1] = fs.psi;
        dst[2] = fs.kap;
    };
    if ((at_bottom && hoist_b) || (at_top && hoist_t && !at_bottom)) // (one divergent pass for both lanes)
        hoist_face(at_bottom ? FACE_BOTTOM : FACE_TOP, at_bottom ? 0 : qt);
    if (at_bottom && at_top && hoist_t) hoist_face(FACE_TOP, qt); // a column of <= CW cells
    wave_sync();
    FT nf_acc = FT(0);
    for (int64_t s = 0; s < nsteps; ++s) {
        FT u_vl[CW], u_re[CW]; // the stage state
#pragma unroll
        for (int q = 0; q < CW; ++q) {
            u_vl[q] = y_vl[q];
            u_re[q] = y_re[q];
        }
#pragma unroll 1
        for (int stage = 0; stage < 3; ++stage) {
            LH_CSW_STAGE_BOUNDARY_VALUES;
            FT T[CW], kap[CW], K[CW], psi[CW], E[CW]; // psi: -psi
#pragma unroll
            for (int q = 0; q < CW; ++q) {
                float dpsi, ircs; // (the step bound's: not formed here)
                cell_closures<FT, M, MODEL, FACTORS, NOICE, false>(mm, P, c, u_vl[q], ti[q], u_re[q], Ta[q], vgf, T[q], kap[q], K[q],
                                                                   psi[q], E[q], dpsi, ircs);
            }
            // the lane's top cell, for the lane above
            if (WATER) { ex.K[l] = K[CW - 1]; ex.h[l] = psi[CW - 1]; }
            if (HEAT) { ex.T[l] = T[CW - 1]; ex.kap[l] = kap[CW - 1]; }
            if (HEAT && WATER) ex.E[l] = E[CW - 1];
            wave_sync();
            // boundary faces: the lane with the bottom cell and the lane with the top cell go through
            // boundary_fluxes TOGETHER (one divergent pass, not two, when both faces need closures)
            FT Fw_b = FT(0), Fe_b = FT(0), Fw_t = FT(0), Fe_t = FT(0);
            if (at_bottom || at_top) {
                // (the top cell's slot qt is uniform: a chain of selects over the unrolled slots)
                FT bv = u_vl[0], bti = ti[0], bT = T[0], bK = K[0], bpsi = psi[0];
                if (!at_bottom) {
#pragma unroll
                    for (int q = 1; q < CW; ++q)
                        if (q == qt) { bv = u_vl[q]; bti = ti[q]; bT = T[q]; bK = K[q]; bpsi = psi[q]; }
                }
                auto face_fluxes = [&](int face, bool hoisted, FT& fe, FT& fw) {
                    FaceState<FT> fs;
                    if (hoisted) {
                        const FT* src = sFace + (face == FACE_BOTTOM ? 0 : 3);
                        fs.K = src[0];
                        fs.psi = src[1];
                        fs.kap = src[2];
                        fs.T = face_state_T<FT, MODEL>(P, face, col, bT);
                    } else {
                        fs = face_state<FT, M, MODEL, FACTORS, NOICE>(mm, P, c, face, col, bv, bti, bT, vgf);
                    }
                    boundary_fluxes_from<FT, MODEL>(P, fs, face, col, bT, bK * Ksc, -bpsi, fe, fw);
                    fe = fe * P.inv_dz;
                    fw = fw * P.inv_dz;
                };
                FT fe, fw;
                face_fluxes(at_bottom ? FACE_BOTTOM : FACE_TOP, at_bottom ? hoist_b : hoist_t, fe, fw);
                if (at_bottom) { Fe_b = fe; Fw_b = fw; }
                else { Fe_t = fe; Fw_t = fw; }
                if (at_bottom && at_top) { // a column of <= CW cells: the same lane owns both faces
#pragma unroll
                    for (int q = 0; q < CW; ++q)
                        if (q == qt) { bv = u_vl[q]; bti = ti[q]; bT = T[q]; bK = K[q]; bpsi = psi[q]; }
                    face_fluxes(FACE_TOP, hoist_t, Fe_t, Fw_t);
                }
            }
            // F[q]: the face below the lane's cell q; F[CW]: the face above its top cell
            FT Fw[CW + 1], Fe[CW + 1];
#pragma unroll
            for (int q = 0; q <= CW; ++q) Fw[q] = Fe[q] = FT(0);
            if (at_bottom) {
                Fw[0] = Fw_b;
                Fe[0] = Fe_b;
            } else { // interior_face's lines, here and below (through the call one instantiation takes other SGPRs)
                FT gh = FT(0);
                if (WATER) {
                    gh = head_difference(psi[0], ex.h[l - 1], P.dz) * cgw;
                    Fw[0] = -(ex.K[l - 1] + K[0]) * gh;
                }
                if (HEAT) {
                    const FT gT = (T[0] - ex.T[l - 1]) * cgT;
                    Fe[0] = -(ex.kap[l - 1] + kap[0]) * gT;
                    if (WATER) Fe[0] = Fe[0] - (ex.E[l - 1] + E[0]) * gh;
                }
            }
#pragma unroll
            for (int q = 1; q < CW; ++q) {
                FT gh = FT(0);
                if (WATER) {
                    gh = head_difference(psi[q], psi[q - 1], P.dz) * cgw;
                    Fw[q] = -(K[q - 1] + K[q]) * gh;
                }
                if (HEAT) {
                    const FT gT = (T[q] - T[q - 1]) * cgT;
                    Fe[q] = -(kap[q - 1] + kap[q]) * gT;
                    if (WATER) Fe[q] = Fe[q] - (E[q - 1] + E[q]) * gh;
                }
            }
            // the face above the lane's top cell is the face below the next lane's bottom cell
            if (WATER) sFw[l] = Fw[0];
            if (HEAT) sFe[l] = Fe[0];
            wave_sync();
            if (l < 63) {
                if (WATER) Fw[CW] = sFw[l + 1];
                if (HEAT) Fe[CW] = sFe[l + 1];
            }
            if (at_top) { // the face above the column's top cell (slot qt) is the boundary
#pragma unroll
                for (int q = 0; q < CW; ++q)
                    if (q == qt) { Fw[q + 1] = Fw_t; Fe[q + 1] = Fe_t; }
            }
#pragma unroll
            for (int q = 0; q < CW; ++q) {
                const FT dvl = WATER ? Fw[q] - Fw[q + 1] : FT(0);
                const FT dre = HEAT ? Fe[q] - Fe[q + 1] : FT(0);
                if (act[q]) {
                    if (WATER) nf_acc = fma_ft(dvl, FT(0), nf_acc);
                    if (HEAT) nf_acc = fma_ft(dre, FT(0), nf_acc);
                }
                if (WATER) u_vl[q] = ssprk33_stage_value<FT>(stage, y_vl[q], u_vl[q], dvl, dt);
                if (HEAT) u_re[q] = ssprk33_stage_value<FT>(stage, y_re[q], u_re[q], dre, dt);
            }
            wave_sync(); // the neighbours have read this stage's LDS values
        }
#pragma unroll
        for (int q = 0; q < CW; ++q) {
            y_vl[q] = u_vl[q];
            y_re[q] = u_re[q];
        }
    }
    if constexpr (BOUND) {
        // The step came from *dt_device (a BOUND launch always has one), which leaves the scalar argument
        // free: it carries the Courant factor, exactly as rhs_kernel MODE 4 takes it.  Named here so that
        // nothing below reads `dt_value` as a step.
        const FT courant = dt_value;
        // (every neighbour has read the last stage's LDS values: the wave_sync that ends a stage)
        FT K[CW], kap[CW], T[CW];
        float dpsi[CW], ircs[CW];
#pragma unroll
        for (int q = 0; q < CW; ++q) {
            FT psi, E; // (not needed by the bound)
            cell_closures<FT, M, MODEL, FACTORS, NOICE, true>(mm, P, c, y_vl[q], ti[q], y_re[q], Ta[q], vgf, T[q], kap[q], K[q], psi, E,
                                                              dpsi[q], ircs[q]);
        }
        // the lane's top cell, for the lane above (a float passes through an FT word unchanged)
        if (WATER) { ex.K[l] = K[CW - 1]; ex.h[l] = FT(dpsi[CW - 1]); }
        if (HEAT) { ex.kap[l] = kap[CW - 1]; ex.T[l] = FT(ircs[CW - 1]); }
        wave_sync();
        float DmaxW = 0.0f, DmaxWb = 0.0f, DmaxT = 0.0f; // as rhs_kernel MODE 4 names them
#pragma unroll
        for (int q = 0; q < CW; ++q) { // the interior face below cell q
            const int i = CW * l + q;
            if (i > 0 && i < n) {
                FT K_p = FT(0), kap_p = FT(0);
                float dpsi_p = 0.0f, ircs_p = 0.0f;
                if (q > 0) { // the cell below is the lane's own (q is a constant of the unrolled loop)
                    K_p = K[q - 1]; kap_p = kap[q - 1]; dpsi_p = dpsi[q - 1]; ircs_p = ircs[q - 1];
                } else {
                    if (WATER) { K_p = ex.K[l - 1]; dpsi_p = float(ex.h[l - 1]); }
                    if (HEAT) { kap_p = ex.kap[l - 1]; ircs_p = float(ex.T[l - 1]); }
                }
                if (WATER) DmaxW = max_nonneg(DmaxW, float(K_p + K[q]) * max_nonneg(dpsi_p, dpsi[q]));
                if (HEAT) DmaxT = max_nonneg(DmaxT, float(kap_p + kap[q]) * max_nonneg(ircs_p, ircs[q]));
            }
        }
        // the boundary cells' own coefficients; Dirichlet faces: half a cell away, face-state coefficients
        auto boundary_terms = [&](int face, bool hoisted, int q_cell) {
            FT bv = y_vl[0], bti = ti[0], bT = T[0], bK = K[0], bkap = kap[0];
            float bdpsi = dpsi[0], bircs = ircs[0];
#pragma unroll
            for (int q = 1; q < CW; ++q)
                if (q == q_cell) { bv = y_vl[q]; bti = ti[q]; bT = T[q]; bK = K[q]; bkap = kap[q]; bdpsi = dpsi[q]; bircs = ircs[q]; }
            FT K_f, kap_f;
            if (hoisted) {
                const FT* src = sFace + (face == FACE_BOTTOM ? 0 : 3);
                K_f = src[0];
                kap_f = src[2];
            } else {
                const FaceState<FT> fs = face_state<FT, M, MODEL, FACTORS, NOICE>(mm, P, c, face, col, bv, bti, bT, vgf);
                K_f = fs.K;
                kap_f = fs.kap;
            }
            const FT K_c = bK * Ksc; // the true conductivity of the boundary cell
            DmaxW = max_nonneg(DmaxW, 2.0f * float(bK) * bdpsi);
            DmaxWb = max_nonneg(DmaxWb, 4.0f * float(fmax_ft(K_f, K_f > FT(0) ? K_c : FT(0))) * bdpsi);
            if (HEAT) {
                DmaxT = max_nonneg(DmaxT, 2.0f * float(bkap) * bircs);
                DmaxT = max_nonneg(DmaxT, 4.0f * float(fmax_ft(kap_f, kap_f > FT(0) ? bkap : FT(0))) * bircs);
            }
        };
        if (at_bottom || at_top) boundary_terms(at_bottom ? FACE_BOTTOM : FACE_TOP, at_bottom ? hoist_b : hoist_t, at_bottom ? 0 : qt);
        if (at_bottom && at_top) boundary_terms(FACE_TOP, hoist_t, qt); // a column of <= CW cells
        // wave maxima (every lane of the wave is here: the kernel has no early exit)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            DmaxW = max_nonneg(DmaxW, __shfl_xor(DmaxW, off, 64));
            DmaxWb = max_nonneg(DmaxWb, __shfl_xor(DmaxWb, off, 64));
            if (HEAT) DmaxT = max_nonneg(DmaxT, __shfl_xor(DmaxT, off, 64));
        }
        if (l == 0 && col_raw < P.ncols) { // (a column whose maximum is NaN is dropped, as in MODE 4)
            const float Dj = max_nonneg(max_nonneg(DmaxW * float(Ksc), DmaxWb) * float(FT(1) / (c.n * c.m)), DmaxT);
            const float dmax = Dj == Dj ? max_nonneg(0.0f, Dj) : 0.0f;
            if (dmax > 0.0f) bound_publish<FT>(P, courant, dmax);
        }
    }
    __syncthreads(); // the tiles overlay other columns' exchange arrays
#pragma unroll
    for (int q = 0; q < CW; ++q) {
        const int i = CW * l + q;
        if (i < n) {
            if (WATER) tiles[slot * n + i] = y_vl[q];
            if (HEAT) tiles[tile_n + slot * n + i] = y_re[q];
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < tile_n; e += blockDim.x) {
        const int lev = e / cpb, cs = e - lev * cpb;
        if (col_first + cs < P.ncols) {
            const int64_t g = int64_t(lev) * P.stride + col_first + cs;
            if (WATER) Y.v[0][g] = tiles[cs * n + lev];
            if (HEAT) Y.v[2][g] = tiles[tile_n + cs * n + lev];
        }
    }
    if (col_raw < P.ncols && nf_acc != nf_acc) atomicOr(P.status, 1u);
