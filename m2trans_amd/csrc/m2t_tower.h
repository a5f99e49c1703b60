// m2t_tower.h -- what the two frozen transformer towers (m2t_swin.hip, m2t_text.hip) share on the host: the resolved offsets of
// one transformer layer (a Swin block or a BERT layer), the helpers that register its parameters and packs in an m2t_layout and
// record the offsets they get, the one-time packing of its weights, and the GEMM wrapper of every pass.  Host code only.
// Names are spelled in m2t_*_create (through the helpers here) and nowhere after it: the passes index these structs.
#pragma once
#include "m2t_kernels.h"
#include "m2t_layout.h"

struct m2t_tower_layer {
  int C, FF;                                               // width, hidden width of the MLP
  long long w[3], b[3];                                    // parameters, offsets in floats: q, k, v weight [C][C] and bias
  long long o_w, o_b, fc1_w, fc1_b, fc2_w, fc2_b;          //   attention output [C][C], fc1 [FF][C], fc2 [C][FF]
  long long pk_qkv, pk_o, pk_fc1, pk_fc2;                  // packs, offsets in elements inside ws "packed": q | k | v fused [3C][C]
  long long fb_qkv;                                        // fused q | k | v bias, offset in floats inside ws "fbias"
};

// the parts of a layer both checkpoints name alike, under the prefix `b`; each tower registers its own LayerNorms (and the Swin
// block its relative-position table) between them, in its checkpoint's order
inline void tower_add_qkv(m2t_layout& lay, const std::string& b, m2t_tower_layer& L) {
  const char* nm[3] = {"query", "key", "value"};
  for (int i = 0; i < 3; ++i) {
    L.w[i] = lay.add_param(b + "attention.self." + nm[i] + ".weight", (long long)L.C * L.C);
    L.b[i] = lay.add_param(b + "attention.self." + nm[i] + ".bias", L.C);
  }
}
inline void tower_add_o(m2t_layout& lay, const std::string& b, m2t_tower_layer& L) {
  L.o_w = lay.add_param(b + "attention.output.dense.weight", (long long)L.C * L.C);
  L.o_b = lay.add_param(b + "attention.output.dense.bias", L.C);
}
inline void tower_add_mlp(m2t_layout& lay, const std::string& b, m2t_tower_layer& L) {
  L.fc1_w = lay.add_param(b + "intermediate.dense.weight", (long long)L.FF * L.C);
  L.fc1_b = lay.add_param(b + "intermediate.dense.bias", L.FF);
  L.fc2_w = lay.add_param(b + "output.dense.weight", (long long)L.C * L.FF);
  L.fc2_b = lay.add_param(b + "output.dense.bias", L.C);
}
inline void tower_add_packs(m2t_layout& lay, const std::string& b, m2t_tower_layer& L) {
  L.pk_qkv = lay.add_pack(b + "qkv", 3LL * L.C * L.C);
  L.pk_o = lay.add_pack(b + "o", (long long)L.C * L.C);
  L.pk_fc1 = lay.add_pack(b + "fc1", (long long)L.FF * L.C);
  L.pk_fc2 = lay.add_pack(b + "fc2", (long long)L.C * L.FF);
  L.fb_qkv = lay.add_fb(b + "qkv_bias", 3 * L.C);
}

// once per weight set: the layer's frozen fp32 weights -> element type `dt` (`esz` bytes) in `packed`, q | k | v fused into one
// matrix and one fp32 bias
inline int tower_pack_layer(int dt, size_t esz, const m2t_tower_layer& L, const float* weights, char* packed, float* fbias, hipStream_t st) {
  const long long CC = (long long)L.C * L.C, FC = (long long)L.FF * L.C;
  for (int i = 0; i < 3; ++i) {
    CK(launch_convert(dt, weights + L.w[i], packed + (L.pk_qkv + i * CC) * esz, CC, st));
    CK(launch_convert(M2T_F32, weights + L.b[i], fbias + L.fb_qkv + i * L.C, L.C, st));
  }
  CK(launch_convert(dt, weights + L.o_w, packed + L.pk_o * esz, CC, st));
  CK(launch_convert(dt, weights + L.fc1_w, packed + L.pk_fc1 * esz, FC, st));
  CK(launch_convert(dt, weights + L.fc2_w, packed + L.pk_fc2 * esz, FC, st));
  return 0;
}

// Y [M][N] = epilogue(A [M][K] . W [N][K]^T); `bias` and `aux` (residual / gelu' operand, row stride N) may be null
inline int tower_gemm(int dt, int emode, const void* A, int K, const void* W, void* Y, int N, long long M, const float* bias,
                      const void* aux, hipStream_t st) {
  m2t_gemm_args ga{};
  ga.A = A; ga.lda = K; ga.W = W; ga.Y = Y; ga.ldy = N; ga.bias = bias; ga.aux = aux; ga.ldaux = N;
  ga.M = M; ga.N = N; ga.K = K; ga.H = 1; ga.Wd = 1; ga.r = 1; ga.C = 64;
  return launch_gemm_nt(dt, M2T_A_PLAIN, emode, ga, st);
}
