"""The operand contract of libsslam_weight.so as a table, as tests/conf_table.py is for libsslam_conf.so: for the entries that take
device pointers, the least alignment in bytes of each pointer argument - what the block "ALIGNMENT" of include/sslam_weight.h
states, line for line - and the size limits - what its block "SIZE LIMITS" states, line for line
(tests/test_weighted_refine_cpu.py compares both and holds the table against sslam_amd.lib.WEIGHT_EXPORTS and the library's
dynamic symbols; tests/test_gpu_weighted_refine.py runs every row at its loosest alignment).  No entry of this library takes a
stride.  No torch, no GPU: importable anywhere.
"""

E_INVALID, E_UNSUPPORTED = -1, -2
MAX_K, CHUNK, THREADS, SUMS = 4096, 1024, 256, 28
WEIGHT_PRODUCT, WEIGHT_EXPECTED_ERROR = 0, 1

# entry -> {pointer argument: least alignment in bytes}, in the header's order
ALIGN = {
    "sslu_match_weights": dict(conf_bank=4, pair_first=4, pair_second=4, matches=8, count=4, weight=4),
    "sslu_pose_refine_weighted_pairs": dict(kp_bank=8, kp_depth_bank=4, pair_first=4, pair_second=4, matches=8, count=4, T_in=8, weight=4, T=8,
                                            status=4, iterations=4, selected_count=4, usable_count=4, inlier_count_in=4, inlier_count=4,
                                            inlier_of_slot=4, cost_in=8, cost=8, rms=8, info=8, weight_sum=8),
}

# entry -> the expressions the dispatch code tests (each with the code returned where it is false), the largest accepted value of
# each limited argument, and the widths in bits of the kernels' index expressions
LIMITS = {
    "sslu_match_weights": dict(limits=[("n_pairs * n1 <= 0x7fffffff", E_UNSUPPORTED)], largest=dict(slots=0x7fffffff),
                               widths={"slot index pair * n1": 64, "frame * K": 64}),
    "sslu_pose_refine_weighted_pairs": dict(limits=[("n1 <= K", E_INVALID), ("K <= 4096", E_UNSUPPORTED)], largest=dict(K=MAX_K, n1=MAX_K),
                                            widths={"pair * n1": 64, "frame * K": 64}),
}

# the entries that take no device pointer
HOST_ONLY = ["sslu_version", "sslu_arch", "sslu_launch_count"]


def header_lines():
    """The ALIGNMENT table as the lines of the header's block: `entry: arg a, arg a, ...`."""
    return [f"{entry}: " + ", ".join(f"{k} {v}" for k, v in args.items()) for entry, args in ALIGN.items()]


def limit_lines():
    """The SIZE LIMITS table as the lines of the header's block."""
    out = []
    for entry, row in LIMITS.items():
        tests = "; ".join(f"{expr}, else {'SSLAM_E_UNSUPPORTED' if code == E_UNSUPPORTED else 'SSLAM_E_INVALID'}" for expr, code in row["limits"])
        out.append(f"{entry}: {tests}. offsets: " + ", ".join(f"{k} {v}" for k, v in row["widths"].items()))
    return out


def static_lds_bytes(weighted=True):
    """The refinement kernel's static LDS: the usable slots (uint16), X_a as three doubles and frame b's keypoint (float2) of the
    chunk, with weights one float more per chunk row, the four waves' partial sums and counts."""
    return 2 * MAX_K + CHUNK * (3 * 8 + 8 + (4 if weighted else 0)) + (THREADS // 64) * SUMS * 8 + (THREADS // 64) * 4
