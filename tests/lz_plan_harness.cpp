// Host harness for csrc/lz_plan.h (tests/test_lz_plan.py), compiled with plain g++ against that header alone.
//   lz_plan_harness switches      one line: lz_switches_read() under the environment the test passed, member by member
//   lz_plan_harness plan FILE     FILE: one case per line, "nblocks num_cu fb of" and the switches in the order of print_switches;
//                                 one line per case: the plan, then the fallback grids of a full batch and of the call's last batch
// With -DMI_MEASURE the three measurement switches are read and printed too (without it their columns are read and ignored).
#include "../compression_algorithms_amd/csrc/lz_plan.h"
#include <cstdio>

static void print_switches(const LzSwitches &sw)
{
    printf("%d %u %d %d %d %d %d %u %d %u %d %d %d %d", (int)sw.v2, sw.batch, (int)sw.no_overlap, (int)sw.b_split, sw.fb2_side,
           (int)sw.prof_fallback, (int)sw.rows, sw.rows_waves, (int)sw.big_split, sw.lanes_kib, (int)sw.prefix, (int)sw.debug,
           (int)sw.lzw_sliced, (int)sw.lzs_serial);
#ifdef MI_MEASURE
    printf(" %d %u %d", sw.skip, sw.stop_phase, (int)sw.unsafe_no_fallback);
#endif
    printf("\n");
}

static void print_grids(const LzPlan &pl, uint32_t nb)
{
    const LzFbGrids g = lz_plan_fallback_grids(pl, nb);
    printf(" %u %u %u %u %u", g.fb_want, g.fgrid, g.giant_cap, g.giant_grid, g.small_grid);
}

int main(int argc, char **argv)
{
    if (argc == 2 && argv[1][0] == 's') { print_switches(lz_switches_read()); return 0; }
    if (argc != 3 || argv[1][0] != 'p') return 2;
    FILE *f = fopen(argv[2], "r");
    if (!f) return 2;
    unsigned long long nblocks;
    unsigned num_cu, fb, of, batch, rows_waves, lanes_kib, stop_phase;
    int v2, no_overlap, b_split, fb2_side, prof, rows, big_split, prefix, debug, sliced, serial, skip, no_fb;
    while (fscanf(f, "%llu %u %u %u %d %u %d %d %d %d %d %u %d %u %d %d %d %d %d %u %d", &nblocks, &num_cu, &fb, &of, &v2, &batch, &no_overlap,
                  &b_split, &fb2_side, &prof, &rows, &rows_waves, &big_split, &lanes_kib, &prefix, &debug, &sliced, &serial, &skip,
                  &stop_phase, &no_fb) == 21) {
        LzSwitches sw{};
        sw.v2 = v2; sw.batch = batch; sw.no_overlap = no_overlap; sw.b_split = b_split; sw.fb2_side = fb2_side; sw.prof_fallback = prof;
        sw.rows = rows; sw.rows_waves = rows_waves; sw.big_split = big_split; sw.lanes_kib = lanes_kib; sw.prefix = prefix;
        sw.debug = debug; sw.lzw_sliced = sliced; sw.lzs_serial = serial;
#ifdef MI_MEASURE
        sw.skip = skip; sw.stop_phase = stop_phase; sw.unsafe_no_fallback = no_fb;
#endif
        const LzPlan pl = lz_plan(nblocks, num_cu, LzHint{fb, of}, sw);
        printf("%u %d %d %d %d %d %d %d %d %d", pl.nbmax, (int)pl.overlap, pl.nsets, (int)pl.solo, (int)pl.fb_busy, (int)pl.odd_chain,
               (int)pl.want_fb2, (int)pl.b_shape, pl.skip, (int)pl.no_fallback);
        const uint64_t tail = nblocks % pl.nbmax;
        print_grids(pl, pl.nbmax);
        print_grids(pl, tail ? (uint32_t)tail : pl.nbmax);
        printf("\n");
    }
    fclose(f);
    return 0;
}
