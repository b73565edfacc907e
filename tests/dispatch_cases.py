"""The dispatch edge table: for every edge of the planner's eligibility predicates (sprintz_amd/csrc/plan.h), the last shape that takes a
kernel and the first that does not, with the kernel families as literals.  Two tiers read it: tests/test_gpu_dispatch.py runs every row
on the GPU and checks bytes, samples and the dispatch counters; tests/test_plan_cpu.py replays the rows through the planner alone."""

# keywords of test_gpu_dispatch.options(): SPRINTZ_OPT_LAT_CHUNKS, _BLK_CHUNKS, _BLK_KERNELS at the library's defaults, _ENC_PAIR at the test
# session's (tests/conftest.py)
OPTION_DEFAULTS = dict(lat=2048, blk_chunks=2049, mask=9, pair=1)

ROW = dict(lat=0, blk_chunks=1, mask=25)               # decode_row.h on every shape it fits, from one chunk on; encode_blk.h
MASK9 = dict(lat=0, blk_chunks=1, mask=9)              # the default mask from one chunk on: decode_row.h where it measured faster
BLK = dict(lat=0, blk_chunks=1, mask=7)                # decode_blk.h, encode_blk.h, encode_blk_uni
ENC = dict(lat=0, blk_chunks=1, mask=1)                # encode_blk.h alone
OLD = dict(lat=0, blk_chunks=0)                        # the lane-per-column kernels alone
DEF = dict()                                           # the library's defaults (workgroup-per-chunk kernels up to 2 048 chunks)
BLK_ENC = dict(enc_blk=1, dense_compact=1)             # encode_blk.h never builds the container itself
LAT_ENC = dict(enc_lat=1, dense_compact=1)             # nor does encode_lat.h
PAIR4 = dict(enc_pair=1, dense_fused=1)                # the two-column encoder on 4 lanes a chunk (5 .. 8 columns) does

CASES = [
    # id, options, codec, esz, ndims, chunk_len, nchunks, encode families (None: not this case's subject), decode family, keywords of roundtrip()
    # ---- decode_row.h: rows of whole dwords, at most 64 of them (U = row bytes / 4), chunks of whole dwords that hold a group, 4-byte
    #      aligned container and output, the delta codec
    ("row u8 D=256: U=64", ROW, "delta", 1, 256, 256 * 32, 6, BLK_ENC, "dec_row", {}),
    ("row u8 D=260: U=65", ROW, "delta", 1, 260, 260 * 32, 6, None, "dec_generic", {}),              # (more than 256 columns: not decode_fast.h's either)
    ("row u8 D=28: rows of 7 dwords", ROW, "delta", 1, 28, 28 * 40, 20, None, "dec_row", {}),
    ("row u8 D=30: rows of 7.5 dwords", ROW, "delta", 1, 30, 30 * 40, 20, None, "dec_generic", {}),  # (1 200-byte chunks: shorter than half of decode_fast.h's ring)
    ("row u8 D=8 chunk 128: 32 dwords", ROW, "delta", 1, 8, 128, 40, None, "dec_row", {}),
    ("row u8 D=8 chunk 130: 32.5 dwords", ROW, "delta", 1, 8, 130, 40, None, "dec_generic", {}),
    ("row chunk = 16 D: one group", ROW, "delta", 1, 32, 16 * 32, 20, BLK_ENC, "dec_row", {}),
    ("row chunk = 15 D: no group", ROW, "delta", 1, 32, 15 * 32, 20, dict(dense_verbatim=1), "dec_verbatim", {}),
    ("row u16 output aligned", ROW, "delta", 2, 8, 1024, 20, None, "dec_row", {}),
    ("row u16 output shifted by one element", ROW, "delta", 2, 8, 1024, 20, None, "dec_generic", dict(out_shift=1)),
    ("row byte-dense container aligned", ROW, "delta", 1, 32, 2048, 20, None, "dec_row", dict(align=1)),
    ("row byte-dense container shifted by one byte", ROW, "delta", 1, 32, 2048, 20, None, "dec_fast", dict(align=1, comp_shift=1)),
    ("row FIRE", ROW, "xff", 1, 32, 2048, 20, None, "dec_fast", {}),
    ("mask 9 u8 D=32: 8 dwords", MASK9, "delta", 1, 32, 2048, 20, None, "dec_row", {}),
    ("mask 9 u8 D=28: 7 dwords", MASK9, "delta", 1, 28, 28 * 64, 20, None, "dec_fast", {}),
    ("mask 9 u16 D=32", MASK9, "delta", 2, 32, 2048, 20, None, "dec_fast", {}),
    # ---- decode_blk.h: rows of whole 16-byte pieces, at most 80 8-bit / 64 16-bit columns, chunks of at least 32 rows, at most 256
    #      (block, piece) tasks a chunk
    ("blk u8 D=80", BLK, "delta", 1, 80, 80 * 64, 12, BLK_ENC, "dec_blk", {}),
    ("blk u8 D=96", BLK, "delta", 1, 96, 96 * 64, 12, BLK_ENC, "dec_fast", {}),
    ("blk u16 D=64", BLK, "delta", 2, 64, 64 * 64, 12, BLK_ENC, "dec_blk", {}),
    ("blk u16 D=72", BLK, "delta", 2, 72, 72 * 64, 12, BLK_ENC, "dec_fast", {}),
    ("blk chunk = 32 D", BLK, "delta", 1, 32, 32 * 32, 12, BLK_ENC, "dec_blk", {}),
    ("blk chunk = 24 D", BLK, "delta", 1, 32, 24 * 32, 12, BLK_ENC, "dec_generic", {}),               # (768-byte chunks: shorter than half of decode_fast.h's ring)
    ("blk u8 D=16, 256 blocks: T=256", BLK, "delta", 1, 16, 16 * 8 * 256, 6, BLK_ENC, "dec_blk", {}),
    ("blk u8 D=16, 257 blocks: T=257", BLK, "delta", 1, 16, 16 * 8 * 257, 6, dict(enc_pair=1, dense_compact=1), "dec_fast", {}),
    # ---- encode_blk.h: rows of whole 16-byte pieces, at most 256 tasks a chunk, a 16-byte aligned source
    ("enc u8 D=16", ENC, "delta", 1, 16, 2048, 12, BLK_ENC, "dec_fast", {}),
    ("enc u8 D=24: rows of 1.5 pieces", ENC, "delta", 1, 24, 24 * 64, 12, dict(enc_pair=1, dense_compact=1), "dec_fast", {}),
    ("enc T=256", ENC, "delta", 1, 16, 16 * 8 * 256, 6, BLK_ENC, "dec_fast", {}),
    ("enc T=257", ENC, "delta", 1, 16, 16 * 8 * 257, 6, dict(enc_pair=1, dense_compact=1), "dec_fast", {}),
    ("enc source aligned, slot path", ENC, "delta", 1, 16, 2048, 12, BLK_ENC, "dec_fast", dict(align=1)),
    ("enc source shifted by 4 bytes", ENC, "delta", 1, 16, 2048, 12, dict(enc_generic=1, dense_compact=1), "dec_fast", dict(align=1, src_shift=4)),
    # ---- decode_lat.h / encode_lat.h on default options: at most 64 columns; at most 2 048 chunks to decode and 3 072 to encode, a third
    #      of each from 17 columns on; chunks of at most 16 KB, and up to what fits 150 KB of LDS for batches of at most 64 chunks
    ("lat D=64", DEF, "xff", 1, 64, 64 * 32, 20, LAT_ENC, "dec_lat", {}),
    ("lat D=65", DEF, "xff", 1, 65, 65 * 32, 20, dict(enc_generic=1, dense_compact=1), "dec_generic", {}),
    ("lat u16 x 8, 2 048 chunks", DEF, "xff", 2, 8, 1024, 2048, LAT_ENC, "dec_lat", {}),
    ("lat u16 x 8, 2 049 chunks", DEF, "xff", 2, 8, 1024, 2049, LAT_ENC, "dec_fast", {}),
    ("lat u16 x 8, 3 072 chunks to encode", DEF, "xff", 2, 8, 256, 3072, LAT_ENC, None, {}),
    ("lat u16 x 8, 3 073 chunks to encode", DEF, "xff", 2, 8, 256, 3073, PAIR4, None, {}),
    ("lat D=32, 682 chunks", DEF, "xff", 1, 32, 1024, 682, LAT_ENC, "dec_lat", {}),
    ("lat D=32, 683 chunks", DEF, "xff", 1, 32, 1024, 683, dict(enc_pair=1, dense_compact=1), "dec_generic", {}),
    ("lat 65 chunks of 16 KB", DEF, "xff", 2, 8, 8192, 65, LAT_ENC, "dec_lat", {}),
    ("lat 65 chunks of 16 KB + 16", DEF, "xff", 2, 8, 8200, 65, PAIR4, "dec_fast", {}),
    ("lat 64 chunks of 16 KB + 16", DEF, "xff", 2, 8, 8200, 64, LAT_ENC, "dec_lat", {}),
    # (the carve of 150 KB = 153 600 bytes: decode_lat.h keeps the stream (its bound + 64), 8 bytes a block of group words, 4 bytes an element of
    #  errors and a word per column and block: 45 680 bytes of uint16 x 8 are 47 808 + 2 896 + 91 408 + 11 440 = 153 552, 16 bytes more 153 808;
    #  encode_lat.h keeps the chunk three times, two words per column and block and the image: 33 088 bytes are 153 472, 33 104 are 153 616)
    ("lat 4 chunks of 45 680 bytes to decode", DEF, "xff", 2, 8, 22840, 4, PAIR4, "dec_lat", {}),
    ("lat 4 chunks of 45 696 bytes to decode", DEF, "xff", 2, 8, 22848, 4, PAIR4, "dec_fast", {}),
    ("lat 4 chunks of 33 088 bytes to encode", DEF, "xff", 2, 8, 16544, 4, LAT_ENC, "dec_lat", {}),
    ("lat 4 chunks of 33 104 bytes to encode", DEF, "xff", 2, 8, 16552, 4, PAIR4, "dec_lat", {}),
    # (48 KB is the limit plan.h's lat_chunk_fits states first; the carve above refuses a chunk long before it: both sides on the older kernels)
    ("lat 4 chunks of 48 KB", DEF, "xff", 2, 8, 24576, 4, PAIR4, "dec_fast", {}),
    ("lat 4 chunks of 48 KB + 16", DEF, "xff", 2, 8, 24584, 4, PAIR4, "dec_fast", {}),
    # ---- decode_fast.h against decode_kernel.h: at most 256 columns, the lanes' group more than half full, chunks of at least half the ring
    ("fast D=256", OLD, "xff", 1, 256, 256 * 64, 6, None, "dec_fast", {}),
    ("fast D=257", OLD, "xff", 1, 257, 257 * 64, 6, None, "dec_generic", {}),
    # (a group less than half full cannot happen: the group is the next power of two, or 64 lanes of 2 / 4 columns)
    ("fast D=33: 33 of 64 lanes", OLD, "xff", 2, 33, 33 * 128, 6, None, "dec_fast", {}),
    ("fast D=32: 32 of 32 lanes", OLD, "xff", 2, 32, 32 * 128, 6, None, "dec_fast", {}),
    # (uint16 x 8: the ring, its apron and the block staging are 1 216 bytes)
    ("fast chunk of 608 bytes: half the ring", OLD, "delta", 2, 8, 304, 20, None, "dec_fast", {}),
    ("fast chunk of 592 bytes", OLD, "delta", 2, 8, 296, 20, None, "dec_generic", {}),
]

# test_gather_rows_edges: esz, ndims, the output's shift in elements behind a 16-byte boundary, family
GATHER_EDGES = [
    (2, 8, 0, "gather_fast"),             # rows of 16 bytes
    (2, 12, 0, "gather_generic"),         # rows of 24 bytes
    (1, 32, 0, "gather_fast"),
    (1, 24, 0, "gather_generic"),
    (2, 8, 1, "gather_generic"),          # the output one element behind a 16-byte boundary
    (1, 32, 8, "gather_generic"),
]
