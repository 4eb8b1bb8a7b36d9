"""Sample extraction from packed GLWE ciphertexts in exact uint64 arithmetic, written from the formula alone (it calls no
library): block j of packed results is coefficient c = j % N of GLWE j // N; as an LWE under the flattened GLWE key its
mask word q N + i is A_q[c - i] for i <= c and -A_q[N + c - i] for i > c, its body B[c]
(extract_lwe_sample_from_glwe_ciphertext, core_crypto/algorithms/glwe_sample_extraction.rs:91-147)."""
import numpy as np

# (N, k) and (first, count) as functions of N: a single row, a full GLWE, a range crossing a GLWE boundary, an unaligned
# start, three GLWEs
SHAPES = [(256, 1), (256, 2), (512, 3), (2048, 1)]
RANGES = [lambda N: (0, 1), lambda N: (0, N), lambda N: (N - 1, 2), lambda N: (3, N + 5), lambda N: (0, 2 * N + 1)]
RANGE_IDS = ["one", "N", "cross", "unaligned", "2N+1"]


def extract_exact(glwes, k, N, first, count):
    """glwes: (G, k+1, N) uint64 with G >= ceil((first + count) / N) -> (count, k N + 1) uint64."""
    glwes = np.asarray(glwes, dtype=np.uint64).reshape(-1, k + 1, N)
    out = np.zeros((count, k * N + 1), dtype=np.uint64)
    i = np.arange(N)
    for r in range(count):
        g, c = divmod(first + r, N)
        a = glwes[g, :k, :]
        unwrapped = a[:, (c - i) % N]                       # i <= c: A_q[c - i]; i > c: A_q[N + c - i]
        with np.errstate(over="ignore"):
            row = np.where(i > c, np.uint64(0) - unwrapped, unwrapped)
        out[r, :k * N] = row.reshape(-1)
        out[r, k * N] = glwes[g, k, c]
    return out


def random_glwes(k, N, first, count, seed):
    """Uniformly random words for exactly the GLWEs the range needs."""
    rng = np.random.default_rng([N, k, first, count, seed])
    return rng.integers(0, 2**64, size=(-(-(first + count) // N), k + 1, N), dtype=np.uint64)
