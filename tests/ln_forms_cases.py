"""The case table of the LayerNorm-backward form tests, shared by tests/test_ln_forms_gpu.py (which runs every row) and
tests/test_ln_forms_cpu.py (which holds every row against a restatement of the dispatch rule and against rcot_ln_bwd_rows), so the two
cannot drift.

Every figure of a row is a LITERAL, worked out by hand from rcot_ln_bwd / ln_bwd_grid of csrc/pointwise.hip:
    wide  = ceil(N / 64) * B >= 512            TX = 16, TY = 16, 64-pixel tiles;  else TX = 4, TY = 64, 16-pixel tiles
    NC    = C / TY if C % TY == 0 and C / TY in (3, 6), else 0 (the generic two-pass form)
    tiles = ceil(N / tile),  gx = min(max(1024 // B, 1), tiles),  trips = ceil(tiles / gx),  rows = gx * B
"""
from collections import namedtuple

Case = namedtuple("Case", "name B C N kernel tiles gx trips rows")

CASES = [
    # ---- wide: ceil(4096 / 64) * 8 = 512 >= 512.  64 tiles, gx = min(128, 64) = 64: one trip, 512 rows
    Case("wide-regs-3", 8, 48, 4096, "ln_bwd_kernel<3, 16>", 64, 64, 1, 512),                # 48 / 16 = 3: registers
    # 96 / 16 = 6: registers.  Also the upper side of the threshold: ceil(N / 64) * B = 512 exactly
    Case("wide-regs-6-threshold-512", 8, 96, 4096, "ln_bwd_kernel<6, 16>", 64, 64, 1, 512),
    Case("wide-generic-12-per-row", 8, 192, 4096, "ln_bwd_kernel<0, 16>", 64, 64, 1, 512),   # 192 / 16 = 12: generic
    Case("wide-generic-c100", 8, 100, 4096, "ln_bwd_kernel<0, 16>", 64, 64, 1, 512),         # 100 % 16 = 4: thread-rows 0..3 take 7 channels, the rest 6
    Case("wide-generic-c8", 8, 8, 4096, "ln_bwd_kernel<0, 16>", 64, 64, 1, 512),             # C < TY: thread-rows 8..15 have no channel
    Case("wide-generic-c512", 8, 512, 4096, "ln_bwd_kernel<0, 16>", 64, 64, 1, 512),         # the cap of sdw[512] / sdb[512]
    # the production shape: 256 tiles on gx = min(128, 256) = 128 -> every workgroup takes two tiles; 1024 rows
    Case("wide-two-trips-production", 8, 96, 16384, "ln_bwd_kernel<6, 16>", 256, 128, 2, 1024),
    # ceil(2112 / 64) = 33 tiles (33 * 32 = 1056 >= 512) on gx = min(32, 33) = 32: workgroup 0 alone takes a second tile (tile 32)
    Case("wide-two-trips-one-workgroup", 32, 96, 2112, "ln_bwd_kernel<6, 16>", 33, 32, 2, 1024),
    # ceil(528 / 64) = 9 tiles (9 * 64 = 576 >= 512), gx = min(16, 9) = 9; tile 8 holds pixels 512..527: 4 live lanes of 16
    Case("wide-ragged-tile", 64, 48, 528, "ln_bwd_kernel<3, 16>", 9, 9, 1, 576),
    # 1024 // 1100 = 0 -> gx = 1; one 64-pixel tile over 32 pixels: lanes 8..15 of every thread-row masked; 1100 rows
    Case("wide-b-above-1024", 1100, 48, 32, "ln_bwd_kernel<3, 16>", 1, 1, 1, 1100),
    # ---- the lower side of the threshold: ceil(4672 / 64) * 7 = 73 * 7 = 511 -> narrow; 96 % 64 != 0 -> generic.
    # 4672 / 16 = 292 tiles on gx = min(146, 292) = 146: two trips; 1022 rows
    Case("threshold-511-narrow", 7, 96, 4672, "ln_bwd_kernel<0, 4>", 292, 146, 2, 1022),
    # ---- narrow
    Case("narrow-regs-3", 2, 192, 256, "ln_bwd_kernel<3, 4>", 16, 16, 1, 32),                # 192 / 64 = 3
    Case("narrow-regs-6", 2, 384, 64, "ln_bwd_kernel<6, 4>", 4, 4, 1, 8),                    # 384 / 64 = 6
    Case("narrow-generic", 2, 96, 256, "ln_bwd_kernel<0, 4>", 16, 16, 1, 32),
    # ceil(4096 / 64) * 5 = 320 < 512; 256 tiles on gx = min(204, 256) = 204: workgroups 0..51 take a second tile; 1020 rows
    Case("narrow-two-trips-generic", 5, 96, 4096, "ln_bwd_kernel<0, 4>", 256, 204, 2, 1020),
    Case("narrow-two-trips-regs-3", 5, 192, 4096, "ln_bwd_kernel<3, 4>", 256, 204, 2, 1020),
    Case("narrow-ragged-20", 2, 48, 20, "ln_bwd_kernel<0, 4>", 2, 2, 1, 4),                  # tile 1: pixels 16..19, one live quad of 4
    Case("narrow-ragged-36", 2, 48, 36, "ln_bwd_kernel<0, 4>", 3, 3, 1, 6),                  # tile 2: pixels 32..35, one live quad of 4
    Case("narrow-smallest", 1, 5, 4, "ln_bwd_kernel<0, 4>", 1, 1, 1, 1),                     # one quad, C < TY: thread-rows 5..63 idle
    # ---- the reducers at their loop boundaries (block_param_reduce_kernel: eight rows per trip while r + 224 < rows, r = row-lane
    # 0..31; ln_param_reduce_kernel: two per trip while r + 32 < rows).  The rows above are 1, 4, 6, 8, 32, 512, 576, 1020, 1022, 1024
    # and 1100; none lies in 225..256 or just above 256.
    # 240 rows: row-lanes 0..15 take one eight-row trip, 16..31 only the tail loop.  3840 / 16 = 240 tiles, gx = min(1024, 240)
    Case("reducer-240-rows", 1, 384, 3840, "ln_bwd_kernel<6, 4>", 240, 240, 1, 240),
    # 258 rows: every row-lane takes one eight-row trip, lanes 0 and 1 a tail row (256, 257).  ceil(1376 / 64) * 3 = 66: narrow;
    # 86 tiles, gx = min(341, 86) = 86
    Case("reducer-258-rows", 3, 192, 1376, "ln_bwd_kernel<3, 4>", 86, 86, 1, 258),
]

IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
