// Prints the nine 29-bit limbs of F29::from_mont256(x) for every 256-bit x given on the command line (64 hex digits, most
// significant first), one line of nine hex words per argument: tests/test_pairing_edges_gpu.py pins with it which limbs a
// chosen canonical input of the C-ABI becomes on the device (the preimage x = t * 32^-1 mod p of a limb pattern t).
#include <cstdio>
#include <cstring>
#include "fp29.h"
using namespace lsa;
int main(int argc, char **argv) {
    for (int a = 1; a < argc; a++) {
        if (strlen(argv[a]) != 64) { printf("bad argument %d\n", a); return 2; }
        Fq x;
        for (int w = 0; w < 8; w++) {
            unsigned v = 0;
            if (sscanf(argv[a] + 8 * (7 - w), "%8x", &v) != 1) { printf("bad argument %d\n", a); return 2; }
            x.l[w] = v;
        }
        const F29 r = F29::from_mont256(x);
        for (int i = 0; i < 9; i++) printf("%08x%c", r.l[i], i == 8 ? '\n' : ' ');
    }
    return 0;
}
