"""Narrow packed GLWE results in exact integers, written from the definition alone (include/fhestr.h, "narrow packed
results"; it calls no library).  For a width 8 <= b <= 32:
    narrow_b(x) = ((x + 2^(63-b)) >> (64-b)) mod 2^b          widen_b(v) = v << (64-b)
A packed list of `held` blocks has G = ceil(held / N) GLWEs [k+1][N]; GLWE g holds m_g = min(N, held - g N) blocks and its
stream is kN + m_g fields of b bits, field f = narrow_b(word f of the GLWE), bit t of the stream = bit t & 63 of u64 word
t >> 6, unused high bits 0.  Stream g starts at word g W, W = ceil((kN + N) b / 64); the last has ceil((kN + m_g) b / 64)."""
import numpy as np

BITS = [8, 13, 16, 21, 31, 32]
HELD = [lambda N: 1, lambda N: N - 1, lambda N: N, lambda N: N + 1, lambda N: 2 * N + 1]
HELD_IDS = ["1", "N-1", "N", "N+1", "2N+1"]


def narrow_word(x, b):
    return ((int(x) + (1 << (63 - b))) >> (64 - b)) % (1 << b)


def widen_word(v, b):
    return int(v) << (64 - b)


def edge_words(b):
    """Words that meet a wrap, a tie and their neighbours, with what they narrow to."""
    return [(2**64 - 1, 0), (2**64 - 2**(63 - b), 0), (2**64 - 2**(63 - b) - 1, 2**b - 1), (2**(63 - b), 1), (2**(63 - b) - 1, 0)]


def blocks_of(N, held, g):
    return min(N, held - g * N)


def stream_words(fields, b):
    return -(-fields * b // 64)


def narrow_len(N, k, held, b):
    if held == 0 or not 8 <= b <= 32:
        return 0
    G = -(-held // N)
    return (G - 1) * stream_words(k * N + N, b) + stream_words(k * N + blocks_of(N, held, G - 1), b)


def narrow_fields(glwes, k, N, held, b):
    """Per GLWE the uint64 array of its kN + m_g narrowed fields (numpy, the same integers as narrow_word)."""
    glwes = np.asarray(glwes, dtype=np.uint64).reshape(-1, (k + 1) * N)
    out = []
    for g in range(-(-held // N)):
        x = glwes[g, :k * N + blocks_of(N, held, g)]
        with np.errstate(over="ignore"):
            out.append((x + np.uint64(1 << (63 - b))) >> np.uint64(64 - b))      # the sum wraps mod 2^64: below 2^b
    return out


def narrow_exact(glwes, k, N, held, b):
    """glwes (G, k+1, N) uint64 -> the narrow list, narrow_len uint64 words.  The stream is assembled as one Python integer
    per GLWE: field f at bits f b .. f b + b - 1."""
    out = np.zeros(narrow_len(N, k, held, b), dtype=np.uint64)
    W = stream_words(k * N + N, b)
    for g, fields in enumerate(narrow_fields(glwes, k, N, held, b)):
        bits = np.zeros(stream_words(len(fields), b) * 64, dtype=np.uint8)
        field_bits = (fields[:, None] >> np.arange(b, dtype=np.uint64)[None, :]) & np.uint64(1)
        bits[:len(fields) * b] = field_bits.reshape(-1)
        words = np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1)
        out[g * W:g * W + len(words)] = words
    return out


def widen_exact(narrow, k, N, held, b):
    """The narrow list -> (G, k+1, N) uint64, the body coefficients that hold no block 0."""
    narrow = np.asarray(narrow, dtype=np.uint64).reshape(-1)
    G, W = -(-held // N), stream_words(k * N + N, b)
    out = np.zeros((G, (k + 1) * N), dtype=np.uint64)
    for g in range(G):
        F = k * N + blocks_of(N, held, g)
        words = narrow[g * W:g * W + stream_words(F, b)]
        bits = np.unpackbits(words.astype("<u8").view(np.uint8), bitorder="little")[:F * b].reshape(F, b).astype(np.uint64)
        fields = (bits << np.arange(b, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
        out[g, :F] = fields << np.uint64(64 - b)
    return out.reshape(G, k + 1, N)


def tail_bits_zero(narrow, k, N, held, b):
    narrow = np.asarray(narrow, dtype=np.uint64).reshape(-1)
    W = stream_words(k * N + N, b)
    for g in range(-(-held // N)):
        used = (k * N + blocks_of(N, held, g)) * b
        if used % 64 and int(narrow[g * W + used // 64]) >> (used % 64):
            return False
    return True


def plant_edges(glwes, k, N, held, b):
    """A copy of glwes with edge_words(b) planted, in turn, at the first and last field of every GLWE and at the fields on
    both sides of every 64-bit boundary of its stream that a field does not straddle or that one does."""
    glwes = np.array(glwes, dtype=np.uint64).reshape(-1, (k + 1) * N)
    edges = [w for w, _ in edge_words(b)]
    for g in range(-(-held // N)):
        F = k * N + blocks_of(N, held, g)
        spots = [0, F - 1]
        for t in range(64, F * b, 64):                      # the field that ends at or straddles bit t, and the next one
            spots += [(t - 1) // b, min(F - 1, (t - 1) // b + 1)]
        for i, f in enumerate(spots):
            glwes[g, f] = np.uint64(edges[(i + g) % len(edges)])
    return glwes.reshape(-1, k + 1, N)


def checksum(words):
    """sum of word_i * (2 i + 1) mod 2^64 (what tests/narrow_main.cpp prints per case): the odd multipliers are invertible,
    so any single changed word and any two swapped words change it."""
    w = np.asarray(words, dtype=np.uint64).reshape(-1)
    with np.errstate(over="ignore"):
        return int((w * (np.arange(w.size, dtype=np.uint64) * np.uint64(2) + np.uint64(1))).sum(dtype=np.uint64))
