// smx_prep.h -- the block streamer of smx_prep.hip for the other model-free entries that read a whole count matrix (smx_pca.hip, smx_rankgroups.hip, smx_mbkmeans.hip): the host
// matrix, dense or CSR, crosses in blocks of rows through one device tile [block][ld] float32, ld = G rounded up to 4, padding zero.  A
// block is a whole number of slices of SMX_PREP_SLICE rows of the GLOBAL row ids, whatever block_rows was asked for.
#pragma once
#include "smx_model.h"

namespace smx {

#define SMX_PREP_SLICE 64                        // rows per partial sum of the per-gene pass

// the host matrix of an entry point and how it is cut into blocks of rows
struct PrepInput {
  const float* x; CsrRows csr; long N; int G; long ld; long block; size_t max_nnz;
};

struct PrepStage {   // the device tile and, for CSR input, the staging of one block
  float* tile = nullptr; int64_t* ptr = nullptr; int32_t* cols = nullptr; float* vals = nullptr;
};

struct GenePart { double* sum; double* sq; int32_t* pos; int32_t* above; };   // each [slices][ld]
struct GeneAcc { double* sum; double* sq; int64_t* pos; int64_t* above; };    // each [ld]

// every refusal of the shared arguments, before any device work (who: the entry's name in the messages)
int prep_check_input(const char* who, const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_cells,
                     int32_t n_genes, int32_t block_rows, int32_t func, const float* row_div, PrepInput* in);
int prep_stage_alloc(DeviceScratch& buf, const PrepInput& in, PrepStage* st, bool want_tile);
// rows [r0, r0 + nb) -> the tile
int prep_load_block(const PrepInput& in, const PrepStage& st, long r0, long nb);
// the per-gene pass of smx_prep_stats over a loaded block: slices of SMX_PREP_SLICE rows summed in row order, then added in slice order
// onto acc, which persists across blocks.  thresh [n_cells] (device) or NULL.
int prep_gene_acc_alloc(DeviceScratch& buf, const PrepInput& in, GenePart* part, GeneAcc* acc);
int prep_launch_gene_sums(const float* tile, long nb, long ld, long r0, const float* thresh, const GenePart& part, const GeneAcc& acc);

}  // namespace smx
