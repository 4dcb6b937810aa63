// ingest_internal.h -- what the ingest units share beside the chunk source: the sequential parse loop (ingest.hip and the
// genome reader's per-chromosome fallback), the context's staging buffers and the FASTA upload of a run that
// loaded its own depth (ingest.hip, ingest_bam.hip).  All three are defined in ingest.hip.
#pragma once
#include "pipeline_internal.h"

namespace rsing __attribute__((visibility("hidden"))) {

void parse_depth_text_host(const char* p, size_t sz, int64_t size, std::vector<int32_t>& rd, rsi_text_stats* st, bool named = false,
                           const std::vector<int32_t>* cols = nullptr, int64_t stride = 0, bool bed = false);
constexpr size_t kTextChunk = size_t(64) << 20;   // bytes of text per transfer + kernel: the size of each staging buffer
int ctx_staging(rsi_ctx* ctx);
int upload_fasta(rsi_ctx* ctx, const uint8_t* fasta, int64_t n);

}  // namespace rsing
