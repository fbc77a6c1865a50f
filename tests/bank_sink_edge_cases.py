"""The banks of tests/test_bank_sink_edges_gpu.py (GPU) and of tests/test_chan_lower_root.py, which checks without a GPU that the
lean kernel takes them and that their first pass has the root arms they are named for."""
IN_RATE = 61_440_000
# name -> ([(rate, centre)], the odd-arm kinds of the first pass's root: "O" plain, "A" alternating)
BANKS = {
    # [0 x 10] | [1 2 1 1 1 1 1 2 0 0] | [1 1]: ends at depth 2, beside the second channel's node
    "all_kinds": ([(48_000, 0), (48_000, -15_000_000), (7_680_000, -19_907_103)], "OA"),
    # the same chain twice [2 1 2 1 1 2 1 2 0 0] | [0 x 10]
    "twins": ([(48_000, 9_000_137), (48_000, 0), (48_000, 9_000_137)], "OA"),
    # [1 1]: ends at depth 2 | [1 1 2 ...]: goes on from that node | [1 2 1 ...]: through its sibling
    "shallow_A": ([(7_680_000, -19_907_103), (48_000, -20_000_000), (48_000, -15_000_000)], "A"),
    # [0 x 10] | [0 0]: ends at depth 2 on the deep channel's path | [0 0 0]
    "centre_O": ([(48_000, 137), (7_680_000, 1_000_000), (3_840_000, 500_000)], "O"),
}
