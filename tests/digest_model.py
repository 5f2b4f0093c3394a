"""csrc/pcm_digest.h restated in numpy: CRC-32 of a WAV payload as field arithmetic in GF(2)[x] / P.

Reflected representation: bit 31 of a word is x^0, "times x" is a right shift with a conditional XOR of 0xEDB88320.
Raw CRC = initial value 0, no final XOR.  One little-endian payload dword d advances a state s to (s ^ d) * x^32, so
the raw CRC of N dwords is sum d_j * x^(32 * (N - j)), and

    zlib(D) = raw(D) ^ 0xFFFFFFFF * x^(8 n) ^ 0xFFFFFFFF          (n = len(D); 0 for the empty payload)

The decomposition (the constants are the kernels'):

    tiles   TILE bytes each, aligned to the END of the payload: the first tile of a stream is the ragged one and the
            bytes in front of the payload read as zero (leading zeros do not change a raw CRC)
    waves   a tile is WAVES regions of 64 * K dwords
    lanes   lane l of a wave takes the region's dwords l, l + 64, ... by Horner's rule acc = acc * x^2048 ^ d
            (the constant multiply through four 256-entry tables), then weighs acc with
            x^(32 + 32 * (63 - l)) * x^(2048 * K * (WAVES - 1 - wave)); the tile's value is the XOR of all of them
    join    a stream's tile values, counted from the END (r = 0 is the last tile), thread j of JOIN taking r = j,
            j + JOIN, ... by Horner with x^(8 * TILE * JOIN), weighed with x^(8 * TILE * j), XORed; then the
            x^(8 n) term by square-and-multiply

Test infrastructure only."""
import numpy as np

POLY = 0xEDB88320
ONE = 0x80000000            # x^0
K = 16                      # dwords per lane and tile
WAVES = 4
TILE = WAVES * 64 * K * 4   # DVDA_CRC_TILE_BYTES
JOIN = 256                  # DVDA_CRC_JOIN_TILES


def mulx(a):
    return (a >> 1) ^ (POLY if a & 1 else 0)


def gfmul(a, b):
    r = 0
    for i in range(32):
        if b & (ONE >> i):
            r ^= a
        a = mulx(a)
    return r


def xpow(e):
    """x^e by square-and-multiply"""
    r, p = ONE, mulx(ONE)
    while e:
        if e & 1:
            r = gfmul(r, p)
        p = gfmul(p, p)
        e >>= 1
    return r


def mul_tables(c):
    """four 256-entry tables: v * c = T[0][v & 255] ^ T[1][v >> 8 & 255] ^ T[2][v >> 16 & 255] ^ T[3][v >> 24]"""
    t = np.zeros((4, 256), np.uint32)
    for k in range(4):
        for b in range(256):
            t[k, b] = gfmul(b << (8 * k), c)
    return t


_X2048 = None


def _tables():
    global _X2048
    if _X2048 is None:
        _X2048 = mul_tables(xpow(2048))
    return _X2048


def mulc(t, v):
    """numpy vector times the tables' constant"""
    v = v.astype(np.uint32)
    return t[0][v & 255] ^ t[1][(v >> 8) & 255] ^ t[2][(v >> 16) & 255] ^ t[3][v >> 24]


def tile_value(tile_bytes):
    """raw CRC of one tile (TILE bytes, zero prefix included) the way a workgroup computes it"""
    assert len(tile_bytes) == TILE
    d = np.frombuffer(tile_bytes, "<u4").reshape(WAVES, K, 64)      # [wave][i][lane]
    t = _tables()
    acc = np.zeros((WAVES, 64), np.uint32)
    for i in range(K):
        acc = mulc(t, acc) ^ d[:, i, :]
    v = 0
    for w in range(WAVES):
        for l in range(64):
            v ^= gfmul(int(acc[w, l]), xpow(32 * (64 * K * (WAVES - 1 - w) + 64 - l)))
    return v


def join(tile_values, nbytes):
    """tile values of one stream, first tile first -> zlib CRC-32"""
    if nbytes == 0:
        return 0
    n_t = len(tile_values)
    step = xpow(8 * TILE * JOIN)
    raw = 0
    for j in range(min(JOIN, n_t)):
        acc = 0
        r = j + ((n_t - 1 - j) // JOIN) * JOIN                       # the furthest tile of this thread
        while r >= 0:
            acc = gfmul(acc, step) ^ tile_values[n_t - 1 - r]
            r -= JOIN
        raw ^= gfmul(acc, xpow(8 * TILE * j))
    return raw ^ gfmul(0xFFFFFFFF, xpow(8 * nbytes)) ^ 0xFFFFFFFF


def crc32(payload):
    """zlib.crc32 of `payload` by the kernels' decomposition"""
    n = len(payload)
    n_t = (n + TILE - 1) // TILE
    padded = bytes(n_t * TILE - n) + bytes(payload)
    return join([tile_value(padded[t * TILE:(t + 1) * TILE]) for t in range(n_t)], n)


def crc32_zeros(n):
    """zlib.crc32 of n zero bytes without the buffer: raw(0...) = 0, the initial value's term alone"""
    return (gfmul(0xFFFFFFFF, xpow(8 * n)) ^ 0xFFFFFFFF) if n else 0


def combine(crc_a, crc_b, len_b):
    """crc(A || B) from the two final values"""
    return gfmul(crc_a, xpow(8 * len_b)) ^ crc_b


def write_signed(v, bits):
    """int32 array -> the unsigned field dvda2wav stores: low bits - 1 bits and a sign bit taken from v < 0"""
    v = np.asarray(v, np.int32)
    low = (1 << (bits - 1)) - 1
    return (v.view(np.uint32) & np.uint32(low)) | np.where(v < 0, np.uint32(1 << (bits - 1)), np.uint32(0))


def wav_payload(planar, bits):
    """int32 [channels, frames] -> payload bytes (frame-major, bits / 8 little-endian bytes per value)"""
    u = write_signed(np.ascontiguousarray(np.asarray(planar, np.int32).T), bits).reshape(-1)
    b = u[:, None] >> (8 * np.arange(bits // 8, dtype=np.uint32))[None, :]
    return (b & 255).astype(np.uint8).tobytes()
