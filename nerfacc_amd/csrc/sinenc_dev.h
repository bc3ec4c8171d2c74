// sinenc_dev.h -- the arithmetic of the sinusoidal encoding's backward that sinenc.hip's kernel and the fused T-NeRF training
// backward (nerf_train.hip) share, so that both form the same bits.  Float32, every operation rounded on its own: the files
// that include it are built with -ffp-contract=off.  Formulas and names: the header of sinenc.hip.
#pragma once

namespace nfa {

// tx_kd = (s_k * a) * (g_sin * cos - g_cos * sin); a = 1.0f when neither var nor freq_weights is given
__device__ __forceinline__ float sin_bwd_tx(float sc, float a, float g_sin, float g_cos, float s, float c)
{
    return (sc * a) * (g_sin * c - g_cos * s);
}

// grad_x[n, d] = ((g_id + tx_0d) + tx_1d) + ..., k ascending in one lane; tx: the L terms of this d, `stride` apart
__device__ __forceinline__ float sin_bwd_sum(float g_id, const float *tx, int L, int stride)
{
    float acc = g_id;
    for (int k = 0; k < L; ++k) acc = acc + tx[k * stride];
    return acc;
}

}  // namespace nfa
