"""The operand contract of libsslam_track.so as a table, as tests/place_table.py is for libsslam_place.so: for the entries that take
device pointers, the least alignment in bytes of each pointer argument - what the block "ALIGNMENT" of include/sslam_track.h
states, line for line - and the size limits - what its block "SIZE LIMITS" states, line for line (tests/test_tracks_cpu.py compares
both and holds the table against sslam_amd.lib.TRACK_EXPORTS and the library's dynamic symbols; tests/test_gpu_tracks.py runs every
row at its loosest alignment).  No entry of this library takes a stride.
No torch, no GPU: importable anywhere.
"""

E_INVALID, E_UNSUPPORTED = -1, -2
MAX_K, SCAN_TILE = 4096, 1024
MAX_NODES = 0x7fffffff

# entry -> {pointer argument: least alignment in bytes}, in the header's order
ALIGN = {
    "sslt_link_pairs": dict(pair_first=4, pair_second=4, matches=8, count=4, mask=4, prev=4, next=4, prev_frame=4, next_frame=4),
    "sslt_track_ids": dict(prev=4, prev_frame=4, workspace=8, track_id=4, age=4, n_tracks=4, root_frame=4, root_slot=4, length=4),
    "sslt_landmarks": dict(kp_bank=4, kp_depth_bank=4, C=8, next=4, next_frame=4, root_frame=4, root_slot=4, n_tracks=4, weight=4, xyz=8,
                           n_obs=4, n_kept=4, status=4, weight_sum=8, rms=8, residual=8, kept=4),
    "sslt_track_step": dict(t=4, next_id=4, prev=4, next=4, prev_frame=4, next_frame=4, track_id=4, age=4, matches=8, count=4, mask=4, first=4,
                            out_track_id=4, out_age=4, n_new=4, status=4),
}
OPTIONAL = {"sslt_link_pairs": ("mask",), "sslt_track_ids": (), "sslt_landmarks": ("weight",), "sslt_track_step": ("mask",)}   # may be NULL

# entry -> the expressions the dispatch code tests (each with the code returned where it is false), the largest accepted value of
# each limited argument, and the widths in bits of the kernels' index expressions
LIMITS = {
    "sslt_link_pairs": dict(limits=[("K <= 4096", E_UNSUPPORTED), ("n_bank * K <= 0x7fffffff", E_UNSUPPORTED)],
                            largest=dict(K=MAX_K, nodes=MAX_NODES),
                            widths={"frame * K + slot": 31, "(pair * n1 + slot) * 2": 64}),
    "sslt_track_ids": dict(limits=[("n_bank * K <= 0x7fffffff", E_UNSUPPORTED)], largest=dict(nodes=MAX_NODES),
                           widths={"frame * K + slot": 31, "workspace words": 64}),
    "sslt_landmarks": dict(limits=[("n_bank * K <= 0x7fffffff", E_UNSUPPORTED)], largest=dict(nodes=MAX_NODES),
                           widths={"frame * K + slot": 31, "(frame * K + slot) * 2": 64, "frame * 12": 64, "track * 3": 64}),
    "sslt_track_step": dict(limits=[("K <= 4096", E_UNSUPPORTED), ("capacity * K <= 0x7fffffff", E_UNSUPPORTED)],
                            largest=dict(K=MAX_K, nodes=MAX_NODES), widths={"frame * K + slot": 31}),
}

# the entries that take no device pointer
HOST_ONLY = ["sslt_version", "sslt_arch", "sslt_launch_count", "sslt_track_workspace_bytes"]


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


def workspace_bytes(n_bank, k):
    n = n_bank * k
    return 20 * n + 4 * ((n + SCAN_TILE - 1) // SCAN_TILE)


def launches(entry, n_bank=1):
    """The kernels one call of `entry` launches."""
    rounds = (n_bank - 1).bit_length()                     # ceil(log2 n_bank)
    return {"sslt_link_pairs": 5, "sslt_track_ids": 5 + rounds, "sslt_landmarks": 2, "sslt_track_step": 1}[entry]
