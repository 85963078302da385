// tools/fr_sparse_host_loop.cc -- the host yardstick of tools/bench_fr_sparse.py: y = M x over CSR arrays on one core, the way
// a libsnark prover evaluates its constraints on the CPU: one Montgomery product (csrc/fp.h's 8 x 32-bit CIOS, the host form of
// the device's Fr) and one modular addition per entry, every coefficient a product.  Built as a shared object by the tool.
#include <stddef.h>
#include <stdint.h>

#include "fp.h"
using namespace lsa;

extern "C" void fr_sparse_host_loop(const void *vals, const uint32_t *cols, const uint64_t *row_ptr, size_t nrows, const void *x, void *out) {
    const Fr *v = (const Fr *)vals, *xs = (const Fr *)x;
    Fr *o = (Fr *)out;
    for (size_t r = 0; r < nrows; r++) {
        Fr acc = Fr::zero();
        for (uint64_t e = row_ptr[r]; e < row_ptr[r + 1]; e++) acc = acc + v[e] * xs[cols[e]];
        o[r] = acc;
    }
}
