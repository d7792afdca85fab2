"""The operand contract of libsslam_place.so as a table, as tests/window_table.py is for libsslam_window.so: for the entries that take
device pointers, the least alignment in bytes of each pointer argument - what the block "ALIGNMENT" of include/sslam_place.h
states, line for line - and the size limits - what its block "SIZE LIMITS" states, line for line (tests/test_place_cpu.py compares
both and holds the table against sslam_amd.lib.PLACE_EXPORTS and the library's dynamic symbols; tests/test_gpu_place.py runs every
row at its loosest alignment).  No entry of this library takes a stride.
No torch, no GPU: importable anywhere.
"""

E_INVALID, E_UNSUPPORTED = -1, -2
MAX_CAPACITY, MAX_K, MAX_PER_FRAME, MAX_SLOTS, FRAMES_PER_GROUP = 4096, 4096, 8, 16, 32
MAX_LOG_CAPACITY = 0x7fffffffffffffff // 168      # at n_slots = 1

# entry -> {pointer argument: least alignment in bytes}, in the header's order
ALIGN = {
    "sslp_place_step": dict(t=4, raw=4, sum=4, desc=4, scores=4, workspace=4, first=4, second=4, sim=4, count=4, status=4, sig=4),
    "sslp_edge_log_step": dict(t=4, log_first=4, log_second=4, log_T=8, log_info=8, slot_first=4, new_T=8, new_info=8, new_status=4,
                               new_inliers=4, logged=4, status=4),
}

# entry -> the expressions the dispatch code tests (each with the code returned where it is false), the largest accepted value of
# each limited argument, and the widths in bits of the kernels' index expressions
LIMITS = {
    "sslp_place_step": dict(limits=[("capacity <= 4096", E_UNSUPPORTED), ("k <= 4096", E_UNSUPPORTED), ("d == 128 or d == 256", E_UNSUPPORTED),
                                    ("per_frame <= 8", E_UNSUPPORTED)],
                            largest=dict(capacity=MAX_CAPACITY, k=MAX_K, d=256, per_frame=MAX_PER_FRAME),
                            widths={"frame * d": 31, "keypoint * d": 31}),
    "sslp_edge_log_step": dict(limits=[("n_slots <= 16", E_UNSUPPORTED), ("capacity <= 0x7fffffffffffffff / 168 / n_slots", E_UNSUPPORTED)],
                               largest=dict(n_slots=MAX_SLOTS, capacity=MAX_LOG_CAPACITY),
                               widths={"(frame * n_slots + slot) * 21": 64}),
}

# the entries that take no device pointer
HOST_ONLY = ["sslp_version", "sslp_arch", "sslp_launch_count", "sslp_place_workspace_bytes"]


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


def workspace_bytes(capacity):
    return 4 * capacity
