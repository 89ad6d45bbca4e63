// Part of learn_fused.hip: what the four seat passes of a seated bank share -- adv_obs_kernel (learn_inputgrad.inc), pgd_obs_kernel
// (learn_pgd.inc), cert_obs_kernel (learn_certify.inc) and lin_obs_kernel (learn_linbound.inc).  SeatHead is the head of their argument
// structs (the host fills and checks it once, seat_pass_launch in learn_fused.hip); the functions below are the prologue of a 16-row
// tile of member k's list.  Each kernel keeps its own mode decision and level-word reads, and everything from its first barrier on.
// jury_obs_kernel (learn_jury.inc) takes the same head and prologue with the group / level fields unused.
// ------------------------------------------------------------------------------------------------------------
struct SeatHead {
    copo_ppo_cfg c;
    const float* theta;
    const float* theta_t;
    int64_t member_stride;
    const int64_t* rows;      // [n_members][cap]
    const int32_t* counts;    // [n_members]
    int64_t cap, n_out;
    const float* obs_src;     // [n_out][in_dim]
    int32_t col_lo, col_hi, n_slots;
    const int32_t* group;     // [n_out / n_slots]
    int32_t n_groups;
    const int32_t* level_of;  // [n_groups][n_members]
    const float* levels;      // [n_levels][the pass's level words]
    int32_t n_levels, n_members;
};

// slot mm of a list of n rows: its row, or -1 where there is none (past the list, or an index outside [0, n_out))
__device__ __forceinline__ int64_t seat_row_at(const SeatHead& h, const int64_t* rows, int64_t n, int64_t mm) {
    if (mm >= n) return -1;
    const int64_t r = rows[mm];
    return r >= 0 && r < h.n_out ? r : -1;
}

// the level index of listed row r under member k, or -1 where its group or the index is out of range
__device__ __forceinline__ int seat_level_at(const SeatHead& h, size_t k, int64_t r) {
    const int g = h.group[r / h.n_slots];
    const int lv = g >= 0 && g < h.n_groups ? h.level_of[(size_t)g * h.n_members + k] : -1;
    return lv >= 0 && lv < h.n_levels ? lv : -1;
}

// the tile's sixteen true observation rows into xs [HT][k1p + 4] (zero beyond in_dim and where there is no row; 128-bit loads where the
// rows allow them) and the two mean rows of W3 into w3s [2][H], by all TH threads of the workgroup
template <int TH>
__device__ __forceinline__ void seat_stage(const SeatHead& h, const int64_t* rows, int64_t n, int64_t m0, const float* theta, int H, float* xs,
                                           float* w3s, int tid) {
    const int K1 = h.c.pol.in_dim, K1P = rowpass_k1p(K1), XP = K1P + 4;
    if ((K1 & 3) == 0 && (reinterpret_cast<uintptr_t>(h.obs_src) & 15) == 0) {
        const int qn = K1P >> 2;
        for (int i = tid; i < HT * qn; i += TH) {
            const int row = i / qn, kk = (i - row * qn) * 4;
            const int64_t r = seat_row_at(h, rows, n, m0 + row);
            const bool ok = r >= 0 && kk < K1;
            const float4 v = *reinterpret_cast<const float4*>(h.obs_src + (size_t)(r < 0 ? 0 : r) * K1 + (kk < K1 ? kk : 0));
            *reinterpret_cast<float4*>(xs + row * XP + kk) = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else {
        for (int i = tid; i < HT * K1P; i += TH) {
            const int row = i / K1P, kk = i - row * K1P;
            const int64_t r = seat_row_at(h, rows, n, m0 + row);
            const bool ok = r >= 0 && kk < K1;
            const float v = h.obs_src[(size_t)(r < 0 ? 0 : r) * K1 + (kk < K1 ? kk : 0)];
            xs[row * XP + kk] = ok ? v : 0.0f;
        }
    }
    for (int i = tid; i < 2 * H; i += TH) w3s[i] = theta[h.c.pol.w3 + i];
}
