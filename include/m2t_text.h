/* m2t_text.h -- the MedCLIP text tower of m2t.h (m2t_text_*), readable stage by stage: the encode call with BertModel's
 * hidden_states as a second output.  A sixteenth header on the same library, under the conventions of m2t.h (extern "C", raw device
 * pointers, a hipStream_t passed as void*, 0 / m2t_status / hipError_t as the result, m2t_last_error_string for the text); the fifteen
 * older headers keep their entries.
 *
 * Together with the "ws:<region>" / "wsn:<region>" keys of m2t_text_query this makes every stage input of the LAST layer and the input
 * of EVERY layer visible after one call: tests/test_gpu_text_stages.py compares each kernel of the tower with fp64 on them. */
#ifndef M2T_TEXT_H
#define M2T_TEXT_H
#include "m2t.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* The encode call of m2t.h -- same arguments, same checks, same kernels, same emb bits -- with one more output.  hidden_out may be NULL: then this
 * IS that call.  Otherwise it is [13][n][len][768] in the plan's element type on the device: the embedding output, then the output
 * of each of the 12 layers (BertModel's hidden_states), each copied device-to-device on `stream` right after the kernel that writes it.
 * No new kernel, no synchronisation beyond the one that call has. */
int m2t_text_encode_ex(m2t_text* p, const int* ids_host, const int* mask_host, int n, int len, float* emb, void* workspace,
                       void* stream, void* hidden_out /* may be NULL */);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
