// Host harness for csrc/defh_size.h (tests/test_defh_size.py): the record size k_defh_lengths hands to the scan, computed by
// the same function from a tally and its code lengths.  Input file: cases of 286 u32 (tally) + 286 u8 (lengths) + 2 pad bytes;
// one line "record_bytes n_tokens" per case, once with the whole alphabet in one call and once as 64 lanes would split it.
#include "../compression_algorithms_amd/csrc/defh_size.h"
#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t hist[DEFH_NSYM];
    uint8_t len[DEFH_NSYM + 2];
    while (fread(hist, 4, DEFH_NSYM, f) == DEFH_NSYM && fread(len, 1, DEFH_NSYM + 2, f) == DEFH_NSYM + 2) {
        uint32_t ntok = 0;
        const uint32_t bits = defh_payload_bits(hist, len, 0u, 1u, &ntok);
        uint32_t lane_bits = 0, lane_ntok = 0;
        for (uint32_t lane = 0; lane < 64u; ++lane) { uint32_t t; lane_bits += defh_payload_bits(hist, len, lane, 64u, &t); lane_ntok += t; }
        if (lane_bits != bits || lane_ntok != ntok) { printf("lanes disagree\n"); return 1; }
        printf("%u %u\n", defh_record_bytes(bits), ntok);
    }
    fclose(f);
    return 0;
}
