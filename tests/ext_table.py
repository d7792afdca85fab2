"""The operand contract of libsslam_ext.so as a table, as tests/loose_table.py is for libsslam_hip.so: for every entry that takes
device pointers, the least alignment in bytes of each pointer argument - what the block "ALIGNMENT" of include/sslam_ext.h states,
line for line (tests/test_subcell_cpu.py compares the two and holds the table against sslam_amd.lib.EXT_EXPORTS and the library's
dynamic symbols; tests/test_gpu_subcell.py runs every row at its loosest).  No entry of this library takes a stride.
No torch, no GPU: importable anywhere.
"""

# entry -> {pointer argument: least alignment in bytes}, in the header's order
ALIGN = {
    "sslx_subcell_keypoints": dict(sal=4, idx=4, kp_xy_sub=8, kp_pixel_sub=8, flags=4),
}

# the entries that take no device pointer
HOST_ONLY = ["sslx_version", "sslx_arch", "sslx_launch_count"]


def header_lines():
    """The table as the lines of the header's block: `entry: arg a, arg a, ...`."""
    return [f"{entry}: " + ", ".join(f"{k} {v}" for k, v in args.items()) for entry, args in ALIGN.items()]
