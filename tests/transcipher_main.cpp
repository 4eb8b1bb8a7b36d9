// csrc/stream_cipher.cpp + csrc/transcipher.cpp under a host sanitizer (tests/test_transcipher_host.py): the whole
// transciphering loop on TRIVIAL ciphertexts -- key bits as rows of zeros with bit * delta in the body, every lookup done
// here in the clear from tc_table_value -- with every buffer on the heap at exactly its size, so that a read or write one
// word past the ring, the key rows, the lookup inputs or the destination string is a report.  Both ciphers, 1 and 3 streams,
// the full warm-up and two calls (11 bytes, then 13: 2 + 2 data rounds, the second one from keystream byte 16).  The blocks
// must equal data xor keystream in the layout of string_to_blocks.  Prints one line per case; any mismatch ends the run
// with a nonzero status.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../fhe-string-bounty_amd/csrc/transcipher.h"

static uint64_t splitmix(uint64_t& z) {
    z += 0x9E3779B97F4A7C15ull;
    uint64_t x = z;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

static int run(const fhe_params_t& p, uint32_t cipher, uint32_t S, uint64_t seed) {
    fhe::TcShape sh;
    if (fhe::tc_shape(p, cipher, S, &sh)) return 1;
    const uint32_t L = fhe::stream_key_bits(cipher), big = sh.big, bpc = fhe::tc_blocks_per_char(sh), values = p.msg_mod * p.carry_mod;
    std::vector<uint8_t> key(L / 8), ivs((size_t)S * L / 8);
    for (auto& b : key) b = (uint8_t)splitmix(seed);
    for (auto& b : ivs) b = (uint8_t)splitmix(seed);
    std::unique_ptr<uint64_t[]> key_rows(new uint64_t[(size_t)L * big]()), ring(new uint64_t[fhe::tc_ring_rows(S) * big]);
    for (uint32_t j = 1; j <= L; j++) key_rows[(size_t)(j - 1) * big + big - 1] = fhe::stream_spec_bit(key.data(), L, j) * sh.delta;
    for (size_t i = 0; i < fhe::tc_ring_rows(S) * big; i++) ring[i] = ~0ull;      // whatever a round reads must have been written
    if (fhe::tc_init(sh, key_rows.get(), ivs.data(), ring.get())) return 1;
    int32_t round = 0;
    auto lookups = [&](uint32_t rows, const uint8_t* data, uint32_t n_bytes, uint32_t m) -> int {
        std::unique_ptr<uint64_t[]> in(new uint64_t[(size_t)S * rows * big]);
        std::unique_ptr<uint32_t[]> tables(new uint32_t[(size_t)S * rows]);
        if (fhe::tc_gather(sh, round, rows, ring.get(), key_rows.get(), ivs.data(), data, n_bytes, m, nullptr, in.get(), tables.get())) return 1;
        uint64_t* slot = ring.get() + fhe::tc_slot_row(S, round) * big;
        for (size_t r = 0; r < (size_t)S * rows; r++) {
            const uint64_t* row = in.get() + r * big;
            for (uint32_t w = 0; w + 1 < big; w++)
                if (row[w]) return 2;                                               // trivial in, trivial out
            const uint64_t v = row[big - 1] / sh.delta;
            if (row[big - 1] % sh.delta || v >= values) return 3;
            memset(slot + r * big, 0, (size_t)big * 8);
            slot[r * big + big - 1] = fhe::tc_table_value(tables[r], (uint32_t)v) * sh.delta;
        }
        round++;
        return 0;
    };
    for (uint32_t r = 0; r < fhe::TC_WARMUP_ROUNDS; r++)
        if (int rc = lookups(fhe::TC_STATE_ROWS, nullptr, 0, 0)) return rc;
    uint64_t first_byte = 0;
    for (uint32_t n_bytes : {11u, 13u}) {
        std::vector<uint8_t> plain((size_t)S * n_bytes), data((size_t)S * n_bytes), ks(n_bytes);
        for (auto& b : plain) b = (uint8_t)splitmix(seed);
        for (uint32_t s = 0; s < S; s++) {
            if (fhe::stream_keystream(cipher, key.data(), ivs.data() + (size_t)s * L / 8, first_byte, ks.data(), n_bytes)) return 1;
            for (uint32_t i = 0; i < n_bytes; i++) data[(size_t)s * n_bytes + i] = plain[(size_t)s * n_bytes + i] ^ ks[i];
        }
        const size_t blocks = (size_t)S * n_bytes * bpc;
        std::unique_ptr<uint64_t[]> out(new uint64_t[blocks * big]);
        for (size_t i = 0; i < blocks * big; i++) out[i] = ~0ull;                   // every block must be written
        for (uint32_t m = 0; m < (n_bytes + 7) / 8; m++) {
            if (int rc = lookups(fhe::TC_DATA_ROWS, data.data(), n_bytes, m)) return rc;
            if (fhe::tc_apply(sh, round - 1, ring.get(), n_bytes, m, out.get())) return 1;
        }
        for (size_t b = 0; b < blocks; b++) {
            const uint64_t want = (plain[b / bpc] >> (sh.bits * (b % bpc))) & (p.msg_mod - 1);
            for (uint32_t w = 0; w + 1 < big; w++)
                if (out[b * big + w]) return 4;
            if (out[b * big + big - 1] != want * sh.delta) return 5;
        }
        first_byte += 8 * ((n_bytes + 7) / 8);
    }
    printf("ok cipher %u streams %u rounds %d\n", cipher, S, round);
    return 0;
}

int main() {
    // TOY_K1 (16 values, 2-bit blocks), a 256-value shape with 4-bit blocks, and the 1-bit and 8-bit shapes W1 and W8 of
    // tests/transcipher_ref.py (8 blocks per character; 8 rows per block and 20 tables); the model accepts all four
    const fhe_params_t shapes[4] = {{16, 1, 256, 10, 2, 4, 4, 4, 4, 1e-12, 1e-15, 0}, {16, 2, 128, 10, 2, 4, 4, 16, 16, 1e-12, 1e-15, 0},
                                    {16, 1, 256, 10, 2, 4, 4, 2, 8, 1e-12, 1e-15, 0}, {16, 3, 512, 20, 1, 4, 4, 256, 1, 1e-12, 1e-15, 0}};
    for (const auto& p : shapes)
        for (uint32_t cipher : {FHE_STREAM_TRIVIUM, FHE_STREAM_KREYVIUM})
            for (uint32_t S : {1u, 3u})
                if (int rc = run(p, cipher, S, 0xC0FFEEull + cipher * 131 + S)) {
                    fprintf(stdout, "FAILED cipher %u streams %u: %d\n", cipher, S, rc);
                    return 1;
                }
    // the refusals touch nothing
    const fhe_params_t four_values = {12, 2, 128, 12, 1, 3, 5, 2, 2, 1e-12, 1e-15, 0};
    if (!fhe::tc_supported(four_values, FHE_STREAM_KREYVIUM) || !fhe::tc_supported(shapes[0], 7)) return 1;
    if (!fhe::stream_keystream(9, nullptr, nullptr, 0, nullptr, 1)) return 1;
    return 0;
}
