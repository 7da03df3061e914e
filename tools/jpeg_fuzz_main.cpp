// jpeg_fuzz_main.cpp -- a stand-alone program around siammask_amd/csrc/jpeg_parse.cpp + jpeg_decode.h (no HIP, no library): the
// parser and the host decode over damaged files, meant to be built with -fsanitize=address,undefined (tests/test_jpeg_host.py does):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DSMK_JPEG_STANDALONE \
//       tools/jpeg_fuzz_main.cpp siammask_amd/csrc/jpeg_parse.cpp -o jpeg_fuzz && ./jpeg_fuzz files.bin
// files.bin: uint32 n, n x uint32 length, then the files' bytes.  Every file runs as it is and in three damaged forms: cut at
// each of 16 evenly spaced lengths (len k / 17, k = 1..16), ONE byte overwritten with a seeded value at 64 seeded positions, and
// 0xFF written at 16 seeded positions.  Every result must be a refusal (1 / 2 from the parser) or a decode that wrote a meta row
// (status 0 or not); an intact file must decode with status 0 unless the parser refuses it.  The copies are heap blocks of exactly
// the damaged length, so a read past the end is the sanitizer's to report.  Exit 0: all of that held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/siammask_hip.h"

static uint32_t rng_state;
static uint32_t rng() { return rng_state = rng_state * 1664525u + 1013904223u; }

static long n_refused, n_status, n_clean;

// -> 0 refused, 1 decoded with a status, 2 decoded clean, -1 anything else
static int run(const uint8_t *src, size_t len) {
    uint8_t *data = (uint8_t *)malloc(len ? len : 1);                 // exactly len bytes: the redzone starts behind them
    memcpy(data, src, len);
    static std::vector<int32_t> seg(512 * 512);
    std::vector<int32_t> desc(32), tables((smk_jpeg_tables_bytes() + 3) / 4);
    int rc = smk_host_jpeg_parse(data, len, desc.data(), tables.data(), tables.size() * 4, seg.data(), seg.size());
    int res = -1;
    if (rc == 1 || rc == 2) {
        res = 0;
    } else if (rc == 0) {
        const int w = desc[0], h = desc[1];
        std::vector<uint8_t> out((size_t)h * w * 3);
        int32_t meta[4] = {-1, -1, -1, -1};
        rc = smk_host_jpeg_decode(data, len, out.data(), 3 * (int64_t)w, h, w, meta);
        if (rc == 0 && meta[1] == h && meta[2] == w && meta[0] >= 0 && meta[0] < 16) res = meta[0] ? 1 : 2;
    }
    free(data);
    (res == 0 ? n_refused : res == 1 ? n_status : n_clean) += res >= 0;
    return res;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1 || n > 4096) return 2;
    std::vector<uint32_t> lens(n);
    if (n && fread(lens.data(), 4, n, f) != n) return 2;
    int bad = 0;
    for (uint32_t i = 0; i < n; ++i) {
        std::vector<uint8_t> file(lens[i]);
        if (fread(file.data(), 1, lens[i], f) != lens[i]) return 2;
        const size_t len = file.size();
        rng_state = 12345u + i;
        const int whole = run(file.data(), len);
        if (whole != 0 && whole != 2) { printf("file %u: intact, result %d\n", i, whole); ++bad; }
        for (int k = 1; k <= 16; ++k)
            if (run(file.data(), len * k / 17) < 0) { printf("file %u: cut at %zu\n", i, len * k / 17); ++bad; }
        for (int k = 0; k < 64 + 16 && len; ++k) {
            std::vector<uint8_t> m(file);
            const size_t pos = rng() % len;
            m[pos] = k < 64 ? (uint8_t)(rng() >> 24) : 0xFF;
            if (run(m.data(), len) < 0) { printf("file %u: byte %zu = %u\n", i, pos, m[pos]); ++bad; }
        }
    }
    fclose(f);
    printf("files %u refused %ld status %ld clean %ld bad %d\n", n, n_refused, n_status, n_clean, bad);
    return bad ? 1 : 0;
}
