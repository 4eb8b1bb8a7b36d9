"""The cast of a block from one client's key to another's in exact integers (test infrastructure; calls no library): the
LWE keyswitch of tests/exact_keyswitch.py at the cast key's geometry -- source k N mask words in, the destination's
k N + 1 (to the big key) or n + 1 (to the small key) words out -- and the sample extraction of tests/exact_extract.py in
front of it for blocks that arrive as packed GLWEs; plus the matrix-core keyswitch's digit-fragment layout, written from
its definition (csrc/ks_mfma_kernels.hip.h), for the byte-for-byte comparison of the two digit kernels."""
import types

import numpy as np

from exact_extract import extract_exact
from exact_keyswitch import ExactKeyswitch, decompose_int, edge_big_cts, edge_ksk, keyswitch_int

U64 = np.uint64
TO_BIG, TO_SMALL = 0, 1


def geometry(src, dst, pair, target):
    """The cast as a keyswitch shape exact_keyswitch.py understands: k N = the source's, n + 1 = the words of a
    keyswitched row, the cast key's (base_log, level)."""
    out_dim = dst.n if target == TO_SMALL else dst.k * dst.N
    return types.SimpleNamespace(k=1, N=src.k * src.N, n=out_dim, ks_base_log=pair[0], ks_level=pair[1])


def cast_exact(src, dst, pair, target, key, cts):
    """(count, src k N + 1) -> (count, out_dim + 1), exact limb products."""
    g = geometry(src, dst, pair, target)
    return ExactKeyswitch(g, np.asarray(key, dtype=U64).reshape(-1))(np.asarray(cts, dtype=U64).reshape(-1, g.N + 1))


def cast_int(src, dst, pair, target, key, ct):
    """One block, Python integers throughout: the definition."""
    return keyswitch_int(geometry(src, dst, pair, target), key, ct)


def cast_packed_exact(src, dst, pair, target, key, glwes, first, count):
    """Blocks first .. first + count - 1 of the source's packed GLWEs: extraction, then the keyswitch."""
    return cast_exact(src, dst, pair, target, key, extract_exact(glwes, src.k, src.N, first, count))


def edge_cts(src, dst, pair, target, rng, count):
    return edge_big_cts(geometry(src, dst, pair, target), rng, count)


def edge_key(src, dst, pair, target, rng):
    return edge_ksk(geometry(src, dst, pair, target), rng)


def digit_fragments(cts, in_dim, base_log, level):
    """The A fragments of a batch: int8 [row tile][step][lane = h * 32 + row % 32][16], slot group 2 step + h holding
    epg = 16 // level whole mask elements with their digits level L first, pad slots and rows past the batch zero."""
    cts = np.asarray(cts, dtype=U64).reshape(-1, in_dim + 1)
    epg = 16 // level
    steps = -(-in_dim // (2 * epg))
    tiles = -(-len(cts) // 32)
    out = np.zeros((tiles, steps, 64, 16), dtype=np.int8)
    for b, ct in enumerate(cts):
        for i in range(in_dim):
            grp, e = divmod(i, epg)
            out[b // 32, grp // 2, (grp % 2) * 32 + b % 32, e * level:(e + 1) * level] = decompose_int(int(ct[i]), base_log, level)
    return out.reshape(-1)
