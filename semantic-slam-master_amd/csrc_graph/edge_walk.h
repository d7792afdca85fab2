// edge_walk.h - the WALK of the assembly of include/sslam_graph.h (NORMAL EQUATIONS), shared by csrc_graph/pose_graph.hip (A on a band in
// the workspace) and csrc_window/window.hip (A as a dense triangle in LDS): one statement of which thread adds which staged word to
// which entry, in which order, so both solvers give the same bits.  Included inside an anonymous namespace, after gauss_newton.h.
//   walk_staged   the staged terms of `cnt` slots (edge_terms.h's 90 words each; sa, sb their nodes, sb < 0: not used) are added
//                 in slot order by four groups of 63 threads: a thread owns one entry position (21 of a diagonal block's lower
//                 triangle, 36 of an off-diagonal block, 6 of g) of the nodes n with n % 4 == its group, so every word of A and g
//                 has one writer and takes its terms in ascending slot order.  entry(row, col), row >= col, is where the solver
//                 keeps that word of A.
//   lane_value    lane t's x, for the back substitutions that sum a row's products in ascending k in one wave.
#pragma once

constexpr int WALK = 63;            // entry positions a walking group owns: 21 diagonal, 36 off-diagonal, 6 of g
constexpr int GROUPS = 4;

// lane t's x, for a t the compiler knows (two v_readlane_b32)
__device__ __forceinline__ double lane_value(double x, int t) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), t), hi = __builtin_amdgcn_readlane(__double2hiint(x), t);
    return __hiloint2double(hi, lo);
}

template <class Entry>
__device__ __forceinline__ void walk_staged(const int *sa, const int *sb, const double *stage, int cnt, int tid, Entry entry, double *gv) {
    const int grp = tid / WALK, pos = tid - grp * WALK;
    if (grp >= GROUPS) return;
#pragma unroll 1
    for (int c = 0; c < cnt; c++) {
        const int eb = sb[c], ea = sa[c];
        if (eb < 0) continue;
        const double *st = stage + c * STAGE;
        const int rb = 6 * (eb - 1), ra = 6 * (ea - 1);
        const bool own_b = (eb & (GROUPS - 1)) == grp, own_a = ea >= 1 && (ea & (GROUPS - 1)) == grp;
        if (pos < 21) {                                  // lower triangle of the diagonal blocks
            int i = 0;
            while (tri_lower(i + 1, 0) <= pos) i++;
            const int j = pos - tri_lower(i, 0);
            if (own_b) {
                double *p = entry(rb + i, rb + j);
                *p = *p + st[S_BB + pos];
            }
            if (own_a) {
                double *p = entry(ra + i, ra + j);
                *p = *p + st[S_AA + pos];
            }
        } else if (pos < 57) {                           // the off-diagonal block (b, a)
            const int q = pos - 21, i = q / 6, j = q - 6 * i;
            if (own_b && ea >= 1) {
                double *p = entry(rb + i, ra + j);
                *p = *p + st[S_BA + q];
            }
        } else {                                         // g
            const int i = pos - 57;
            if (own_b) gv[rb + i] = gv[rb + i] + st[S_GB + i];
            if (own_a) gv[ra + i] = gv[ra + i] + st[S_GA + i];
        }
    }
}
