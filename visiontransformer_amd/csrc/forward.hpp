// The forward walk of the model, shared by inference (vitseg_api.hip) and the training step's forward (vitseg_train.hip):
// embeddings, then per layer LN1 -> QKV -> attention -> o_proj + residual -> LN2 -> fc1 + GELU -> fc2 + residual, then the
// final LayerNorm, the 3x3 + 1x1 head and the upsample.  One walk per route (forward.hip): walk_large on the large-batch
// kernels, walk_small on the small-batch route (small.hpp).  The callers say where the tensors live, which dropout applies,
// and the few choices that differ between inference and training (the fields of Fwd below).
#pragma once
#include <functional>

#include "plan.hpp"
#include "small.hpp"

namespace vitseg {

// Where one layer's activations live.  Inference reuses one set for every layer (xin = xmid = xout, ctx in h1's buffer,
// lse / upre / dropw null); training keeps a block per layer for the backward.
struct LayerIO {
    float* xin;            // residual stream entering the layer
    void* h1;              // LayerNorm 1 output (the QKV operand)
    void* qkv;
    void* ctx;             // attention context (o_proj's operand)
    float* lse;            // training: the attention's log-sum-exp per query
    float* xmid;           // residual stream after the attention branch
    void* h2;              // LayerNorm 2 output (fc1's operand)
    void* upre;            // training: fc1's saved pre-activation (GemmArgs::aux / SGemm::aux)
    void* uact;            // MLP hidden (fc2's operand)
    float* xout;           // residual stream leaving the layer
    const unsigned* dropw; // bf16 training: this layer's attention keep-bit words (launch_attn_dropmask), or null
};

// Profile kinds recorded per step (VITSEG_K_*; -1 = no scope).  Inference times each launch group; training only its GEMMs and
// attention.
struct FwdProf {
    int patch, ln, qkv, attn, oproj, fc1, fc2, conv3, head1x1, upsample;
    bool mlp_one_scope;   // large route: fc1 and fc2 under one scope of kind fc1 (the training step's record of them)
};

struct Fwd {
    plan::Shape s;         // the activations' shape (the input's grid)
    const plan::Layout* lay;   // the arena's layout
    const float* params;
    const void* params_lp; // the 16-bit arena (h16), the pre-split one (x3 == 2), or null
    const float* pos;      // the position table the embeddings add (the arena's or its resampled copy)
    const float* x;        // the NCHW images
    int batch;
    float eps;
    hipStream_t st;
    int h16;               // operands of the linears and attention: 0 fp32, 1 bf16, 2 fp16 (and the LayerNorm outputs that feed them)
    int x3;                // large route, VITSEG_F32X3: 1 split operands, 2 weights pre-split (params_lp)
    std::function<LayerIO(int)> layer;
    void* hf;              // final LayerNorm output (the head's input)
    float* F;              // the head's ReLU'd mid features (large route; small route with head_one_chain)
    float* Z;              // low-res logits
    const void* zeros;     // 256-byte zero page (16-bit 3x3 head conv), or null
    float* scratch;        // small route: the K-chunk slabs; large route: split-K partials (GemmArgs::thin_scratch)
    size_t scratch_floats;
    float* logits;         // optional outputs (upsampled logits / argmax mask)
    uint8_t* mask;
    // Dropout with probability drop_p at every (layer, site) (drop_args): training only.
    float drop_p;
    unsigned drop_seed;
    // Large route: the CLS rows of the linears through the split-K side launch when the patch rows are whole row tiles
    // (bitwise batch-invariant: a CLS row takes that path at every batch).  Inference and bf16 training; fp32 training keeps
    // them in the last row tile (the side launch sums their K slices in another order: other bits).
    bool thin_rows;
    // Large route: the scratch goes to every GEMM, so small ones may run whole through K slices (GemmArgs::thin_scratch,
    // whole_split): inference.  Training lends it only with the CLS side launch.
    bool whole_split;
    // bf16 training: fc1 on launch_gemm_bf16_train, which saves the pre-activation for the backward's dGELU.
    bool fc1_train;
    // Small route, the sequence lengths that take the key-split attention kernel: attn_small_infer (inference) or
    // attn_small_train (training: the lengths its backward pair takes).
    bool (*attn_small)(int Np);
    // Small route, the 3x3 head conv as ONE fmaf chain per output in the implicit GEMM's k order (training): its ReLU mask
    // must not depend on a summation order.  Off: nine tap slabs + launch_headfin (inference).
    bool head_one_chain;
    // Large route, fp32: the 3x3 head conv on the LDS-DMA kernel when the conv_dma switch is on (inference only).
    bool conv_dma;
    FwdProf prof;
};

int walk_large(const Fwd& f);
int walk_small(const Fwd& f);

// Slab floats the small route needs (its K-chunk slabs and the head's tap slabs) for Mt token rows, Mp patch rows.
enum SmallRole { SMALL_INFER, SMALL_TRAIN_FWD, SMALL_TRAIN_BWD };
size_t small_slab_floats(const plan::Shape& s, size_t Mt, size_t Mp, SmallRole role);

// CLS rows of the large route's linears that take the split-K side launch (GemmArgs::thin_rows): the batch when the patch
// rows are whole 256-row tiles, else 0
inline int thin_cls_rows(size_t Mp, int batch) { return Mp % 256 == 0 && batch <= THIN_MAX_ROWS ? batch : 0; }

}  // namespace vitseg
