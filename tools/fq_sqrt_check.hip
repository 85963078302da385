// tools/fq_sqrt_check.hip -- the device compilation of csrc/fq_sqrt.h against its host compilation: fq_sqrt, fq2_sqrt and
// g2_in_subgroup over the operand list of tests/cpp/fq_sqrt_cases.h (the list tests/cpp/test_fq_sqrt.cc checks on the host
// against Euler's criterion and [r]P == O), one lane per operand, verdicts and root words compared one for one.  The a1 == 0
// branches of fq2_sqrt cannot be reached through curve points (that would take a cube root in Fq2), so this is where they run
// on the device.  A stand-alone program: no symbol is added to the library.  Built by `make ../fq_sqrt_check` in
// legosnark_amd/csrc (outside `all`), run by tests/test_fq_sqrt_gpu.py.
#include <hip/hip_runtime.h>
#include <string.h>
#include "fq_sqrt_cases.h"

using namespace lsa;

#define HIP_OK(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) { printf("FAIL %s: %s (line %d)\n", #e, hipGetErrorString(e_), __LINE__); return 2; } } while (0)

struct FqRes { Fq root, inv; uint32_t ok; };
struct Fq2Res { Fq2 root; uint32_t ok; };

__global__ __launch_bounds__(256) void k_fq_sqrt(const Fq *in, size_t n, FqRes *out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    FqRes r;
    r.ok = fq_sqrt(in[i], &r.root, &r.inv);
    out[i] = r;
}
__global__ __launch_bounds__(256) void k_fq2_sqrt(const Fq2 *in, size_t n, Fq2Res *out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Fq2Res r;
    r.ok = fq2_sqrt(in[i], &r.root);
    out[i] = r;
}
__global__ __launch_bounds__(256) void k_in_subgroup(const Jac<Fq2> *in, size_t n, uint32_t *out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = g2_in_subgroup(in[i]);
}

template <class In, class Out, class Kernel>
static int run(Kernel k, const std::vector<In> &in, std::vector<Out> &out) {
    const size_t n = in.size();
    out.resize(n);
    In *d_in = nullptr;
    Out *d_out = nullptr;
    HIP_OK(hipMalloc(&d_in, n * sizeof(In)));
    HIP_OK(hipMalloc(&d_out, n * sizeof(Out)));
    HIP_OK(hipMemcpy(d_in, in.data(), n * sizeof(In), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const In *)d_in, n, d_out);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(out.data(), d_out, n * sizeof(Out), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_in));
    HIP_OK(hipFree(d_out));
    return 0;
}

int main() {
    const fqcases::Cases c = fqcases::build(3000);
    int rc;
    size_t bad = 0, accepted = 0;
    {
        std::vector<FqRes> out;
        if ((rc = run(k_fq_sqrt, c.fq, out))) return rc;
        for (size_t i = 0; i < c.fq.size(); i++) {
            Fq root, inv;
            const bool ok = fq_sqrt(c.fq[i], &root, &inv);
            accepted += ok;
            if ((out[i].ok != 0) != ok || !(out[i].root == root) || !(out[i].inv == inv)) { if (!bad++) printf("FAIL fq_sqrt: operand %zu\n", i); }
        }
        printf("fq_sqrt: %zu operands, %zu accepted: verdicts or words differ in %zu\n", c.fq.size(), accepted, bad);
    }
    size_t bad2 = 0, accepted2 = 0, a1zero = 0;
    {
        std::vector<Fq2Res> out;
        if ((rc = run(k_fq2_sqrt, c.fq2, out))) return rc;
        for (size_t i = 0; i < c.fq2.size(); i++) {
            Fq2 root;
            const bool ok = fq2_sqrt(c.fq2[i], &root);
            accepted2 += ok;
            a1zero += c.fq2[i].c1.is_zero();
            if ((out[i].ok != 0) != ok || !(out[i].root == root)) { if (!bad2++) printf("FAIL fq2_sqrt: operand %zu\n", i); }
        }
        printf("fq2_sqrt: %zu operands (%zu with a1 == 0, %zu taking the second candidate), %zu accepted: verdicts or words differ in %zu\n", c.fq2.size(), a1zero,
               c.fq2_second, accepted2, bad2);
    }
    size_t bad3 = 0, in = 0;
    {
        std::vector<uint32_t> out;
        if ((rc = run(k_in_subgroup, c.pts, out))) return rc;
        for (size_t i = 0; i < c.pts.size(); i++) {
            const bool ok = g2_in_subgroup(c.pts[i]);
            in += ok;
            if ((out[i] != 0) != ok) { if (!bad3++) printf("FAIL g2_in_subgroup: point %zu\n", i); }
        }
        printf("g2_in_subgroup: %zu points, %zu in G2: verdicts differ in %zu\n", c.pts.size(), in, bad3);
    }
    if (bad || bad2 || bad3) return 1;
    printf("PASS\n");
    return 0;
}
