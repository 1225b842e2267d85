// tests/test_tile_map_host.py: pgslam_amd/csrc/tile_map.hpp on the host -- the map from a fast-matcher block to its tile.
//   tile_map_host            every (nb, G) of the test's table, four properties each; prints "tile map ok: N cases"
//   tile_map_host dump nb G  the map itself, one tile per line (the Python side checks one case by hand)
#include "tile_map.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

// the contiguous spans as kernels.hip states them (xcd_tile), restated here: the reference the G <= 0 / G >= nb / 8 cases must equal
static int spans(int b, int nb)
{
    const int q = nb >> 3, r = nb & 7;
    const int xcd = b & 7, j = b >> 3;
    return xcd * q + (xcd < r ? xcd : r) + j;
}

static int check(int nb, int G)
{
    std::vector<int> hits((size_t)nb, 0), last(8, -1), count(8, 0);
    for (int b = 0; b < nb; ++b) {
        const int t = pgicp::tile_of_block(b, nb, G);
        if (t < 0 || t >= nb) { std::printf("nb %d G %d: block %d -> tile %d out of range\n", nb, G, b, t); return 1; }
        if (hits[(size_t)t]++) { std::printf("nb %d G %d: tile %d taken twice (block %d)\n", nb, G, t, b); return 1; }
        const int x = b & 7;                                  // blocks of a class arrive in ascending j = b >> 3
        if (t <= last[x]) { std::printf("nb %d G %d: class %d does not ascend at block %d (%d after %d)\n", nb, G, x, b, t, last[x]); return 1; }
        last[x] = t;
        ++count[x];
        if ((G <= 0 || G >= nb / 8) && t != spans(b, nb)) { std::printf("nb %d G %d: block %d -> %d, the spans give %d\n", nb, G, b, t, spans(b, nb)); return 1; }
    }
    for (int t = 0; t < nb; ++t)
        if (hits[(size_t)t] != 1) { std::printf("nb %d G %d: tile %d never taken\n", nb, G, t); return 1; }
    for (int x = 0; x < 8; ++x)
        if (count[x] > (nb + 7) / 8) { std::printf("nb %d G %d: class %d holds %d tiles\n", nb, G, x, count[x]); return 1; }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && argv[1][0] == 'd') {
        const int nb = std::atoi(argv[2]), G = std::atoi(argv[3]);
        for (int b = 0; b < nb; ++b) std::printf("%d\n", pgicp::tile_of_block(b, nb, G));
        return 0;
    }
    std::vector<int> nbs;
    for (int nb = 1; nb <= 70; ++nb) nbs.push_back(nb);
    for (int nb : {128, 512, 1568, 1569, 4093}) nbs.push_back(nb);
    const int groups[] = {-1, 0, 1, 2, 3, 4, 16, 32, 196, 1000};
    int cases = 0;
    for (int nb : nbs)
        for (int G : groups) {
            if (check(nb, G)) return 1;
            ++cases;
        }
    std::printf("tile map ok: %d cases\n", cases);
    return 0;
}
