// gate.h -- the gate of the reference's Adapter (adapter.py:124-179): a row is scaled by base * sigmoid(gate_T * c), c the
// cosine of the row to its NEAREST gate embedding.  The backward's coefficients, one definition for the encoder / decoder
// adapter (csrc/adapter.hip) and the CET text adapter (csrc/cet.hip).  Everything here is internal linkage.
//
// What this pins: the products associate as written.  Its inputs come from divides and roots that are the CORRECTLY ROUNDED
// ones -- both users are built with -fhip-fp32-correctly-rounded-divide-sqrt (build.py), and this header relies on it.
// (The forward's pick -- cosines, first arg-max on a tie, sigmoid -- stays spelled in both kernels: moved into a function here,
// cet_fwd's compares of g against G came out unsigned.)
#ifndef ZIRA_GATE_H_
#define ZIRA_GATE_H_

#include <hip/hip_runtime.h>

namespace {

// With g_c = d loss / d cosine of a row, c its cosine, rn = 1 / |x| and gi = 1 / |gate[amax]|, gs = gate[amax] * gi:
//     g_x    += a * gs + b * x          g_gate[amax] += alpha * x + beta * gs
struct GateCoeffs {
    float a, b, alpha, beta;
};
__device__ __forceinline__ GateCoeffs gate_backward_coeffs(float g_c, float c, float rn, float gi)
{
    GateCoeffs k;
    k.a = g_c * rn;
    k.b = -(g_c * c) * rn * rn;
    k.alpha = g_c * rn * gi;
    k.beta = -(g_c * c) * gi;
    return k;
}

}  // namespace

#endif  // ZIRA_GATE_H_
