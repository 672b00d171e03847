// staged_extract.cc -- the host-staged feature path: arch6 without `gpu_extract` (the reference's SGNN mode).
// Citations are relative to the reference's samgraph/common/.
//
// Reference, cache > 0: DoArch6GetCacheMissIndex + DoCacheIdCopyToCPU + DoArch6CacheFeatureCopy (dist_loops.cc:1015-1207:
// split on the GPU, miss ids to the host, ExtractMissData on the CPU, ONE H2D copy, CombineMissData, CombineCacheData --
// every phase behind a StreamSync); cache 0: DoIdCopy + DoCPUFeatureExtract + DoFeatureCopy (dist_loops.cc:481-583,
// dist_loops_arch6.cc:111-133).  Same data flow here, as a pipeline:
//   * the split is enqueued right behind the sampler with the batch size left on the device
//     (ggms_get_miss_cache_index_dev), the hit rows are combined from the cache shards while the host works;
//   * the miss rows go through pinned memory (hipHostMalloc) in CHUNKS: the host team gathers chunk k + 1 while chunk k's
//     asynchronous H2D copy and its scatter into the batch run -- the copy engine, the combine kernel and the cores
//     overlap instead of taking turns, and the last chunks of batch k overlap the first of batch k + 1;
//   * cache 0: every row is a miss and lands where it belongs -- chunks are copied straight into the batch's feature
//     buffer, no split and no combine;
//   * two short host waits per batch (sizes, miss ids) instead of one per phase.
// `staged_serial_epochs` / `staged_serial_steps` (config keys: the first N epochs / batches) or SAMGRAPH_STAGED_SERIAL=1:
// the reference's serial sequence instead, every phase
// timed behind its own wait and logged under the reference's items (kLogL3CacheExtractMissTime ...): the per-phase
// rates of study/host-extract-speed-amount/data.dat are measured this way.
#include "engine.h"
#include "team.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <thread>
#include <vector>

namespace sam {

// one row into pinned memory: streaming stores (no read-for-ownership of a buffer the CPU never reads back)
static inline void copy_row_stream(char *dst, const char *src, size_t bytes) {
  typedef long long v2di __attribute__((vector_size(16), aligned(1)));
  typedef long long v2da __attribute__((vector_size(16)));
  size_t i = 0;
  if (((uintptr_t)dst & 15) == 0)
    for (; i + 16 <= bytes; i += 16) __builtin_nontemporal_store(*(const v2di *)(src + i), (v2da *)(dst + i));
  if (i < bytes) std::memcpy(dst + i, src + i, bytes - i);
}

static inline void store_fence() { // streaming stores are weakly ordered: drain them before the DMA engine is told to read
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
  asm volatile("sfence" ::: "memory");
#else
  std::atomic_thread_fence(std::memory_order_seq_cst);
#endif
}

void Engine::HostGatherRows(char *rows, const uint32_t *ids, size_t first, size_t count) {
  const char *feat = (const char *)ds.feat.ptr;
  const size_t row_bytes = ds.feat_row_bytes();
  const uint32_t mask = ds.feat_mask;
  host_team_->ParallelFor(count, [&](size_t lo, size_t hi, int) { // ExtractMissData, cuda_cache_manager_host.cc:268-300
    constexpr size_t kAhead = 8; // rows: a random 512-byte row is 8 cache lines nobody has asked for yet
    for (size_t i = lo; i < hi; ++i) {
      if (i + kAhead < hi) {
        const char *nx = feat + (size_t)(ids[first + i + kAhead] & mask) * row_bytes;
        for (size_t o = 0; o < row_bytes; o += 64) __builtin_prefetch(nx + o, 0, 0);
      }
      copy_row_stream(rows + (first + i) * row_bytes, feat + (size_t)(ids[first + i] & mask) * row_bytes, row_bytes);
    }
    store_fence();
  });
}

void Engine::StagedExtract(Batch *b, hipStream_t ss, hipStream_t xs) {
  const uint32_t L = (uint32_t)cfg.fanout.size();
  const size_t row_bytes = ds.feat_row_bytes();
  if (!host_team_) {
    host_team_ = std::make_unique<Team>((int)std::max<size_t>(1, cfg.omp_thread_num));
    log_info("staged extract: host team of " + std::to_string(host_team_->size()) + " threads (omp_thread_num)");
  }
  static const bool env_serial = getenv("SAMGRAPH_STAGED_SERIAL") != nullptr;
  const bool serial = env_serial || cur_epoch_ < cfg.staged_serial_epochs || staged_batches_ < cfg.staged_serial_steps;
  ++staged_batches_;
  const bool have_cache = cache_table_ != nullptr;
  uint64_t *cd = b->trainer.counts_dev;
  uint64_t *n_in = cd + GGMS_COUNT_INPUT(L), *n_miss = cd + GGMS_COUNT_MISS(L), *n_hit = cd + GGMS_COUNT_STAGED_HIT(L);
  using clk = std::chrono::steady_clock;
  auto since = [](clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); };
  double t_index = 0, t_ids = 0, t_gather = 0, t_copy = 0, t_comb_miss = 0, t_comb_hit = 0;
  auto t0 = clk::now();
  // 0. split (GetMissCacheIndex) behind the sampler ON THE BATCH'S SAMPLING STREAM, sizes to the host: wait 1.  The
  // extract stream may still be copying the previous batch's last chunks down -- the cores must not wait for that
  if (have_cache)
    SAM_GGMS(ggms_get_miss_cache_index_dev(cache_table_, b->trainer.input_nodes, max_unique_, n_in, b->miss_src, b->miss_dst, n_miss,
                                           b->hit_src, b->hit_dst, n_hit, b->idx_ws,
                                           ggms_cache_index_workspace_bytes(max_unique_), ss));
  SAM_HIP(hipMemcpyAsync(b->counts, b->trainer.counts_dev, CountsBytes(L), hipMemcpyDeviceToHost, ss));
  SAM_HIP(hipStreamSynchronize(ss));
  const size_t num_input = b->counts[GGMS_COUNT_INPUT(L)];
  size_t num_miss = have_cache ? b->counts[GGMS_COUNT_MISS(L)] : num_input;
  size_t num_hit = have_cache ? b->counts[GGMS_COUNT_STAGED_HIT(L)] : 0;
  if (!have_cache) { // every row comes from the host tier: the counters say so too
    b->counts[GGMS_COUNT_MISS(L)] = num_input;
    SAM_HIP(hipMemcpyAsync(n_miss, b->counts + GGMS_COUNT_MISS(L), 8, hipMemcpyHostToDevice, ss));
  }
  SAM_CHECK(num_miss + num_hit == num_input, "CHECK_EQ(num_miss + num_cache, num_input), dist_loops.cc:1047");
  t_index = since(t0);
  if (num_input == 0) return;
  // 1. miss ids to the host (DoCacheIdCopyToCPU / DoIdCopy): wait 2 -- the hit rows are combined meanwhile
  const uint32_t *ids_dev = have_cache ? b->miss_src : b->trainer.input_nodes;
  t0 = clk::now();
  if (num_miss) SAM_HIP(hipMemcpyAsync(b->miss_ids_host, ids_dev, num_miss * 4, hipMemcpyDeviceToHost, ss));
  SAM_HIP(hipEventRecord(b->ev_ids, ss));
  SAM_HIP(hipStreamWaitEvent(xs, b->ev_ids, 0)); // the extract stream's work of this batch starts behind the split
  auto combine_hits = [&] { // CombineCacheData
    if (!num_hit) return;
    if (num_cache_part_ == 0)
      SAM_GGMS(ggms_gather_scatter(b->feat, cache_parts_[0], b->hit_src, b->hit_dst, num_hit, nullptr, ds.feat_dim,
                                   ds.feat_dtype, xs));
    else
      SAM_GGMS(ggms_gather_scatter_partition(b->feat, (const void *const *)cache_parts_.data(), num_cache_part_, b->hit_src,
                                             b->hit_dst, num_hit, nullptr, ds.feat_dim, ds.feat_dtype, xs));
  };
  if (!serial) combine_hits(); // on the GPU while the cores gather
  SAM_HIP(hipEventSynchronize(b->ev_ids));
  t_ids = since(t0);
  char *rows = (char *)b->miss_rows_host;
  // where a chunk of miss rows lands on the device: the staging area (scattered by CombineMissData), or -- no cache,
  // rows in batch order -- the batch's feature buffer itself
  char *land = have_cache ? (char *)b->miss_rows_dev : (char *)b->feat;
  if (serial) { // the reference's sequence, one phase at a time
    t0 = clk::now();
    HostGatherRows(rows, b->miss_ids_host, 0, num_miss);
    t_gather = since(t0);
    t0 = clk::now();
    if (num_miss) SAM_HIP(hipMemcpyAsync(land, rows, num_miss * row_bytes, hipMemcpyHostToDevice, xs));
    SAM_HIP(hipStreamSynchronize(xs));
    t_copy = since(t0);
    t0 = clk::now();
    if (have_cache && num_miss)
      SAM_GGMS(ggms_gather_scatter(b->feat, b->miss_rows_dev, nullptr, b->miss_dst, num_miss, nullptr, ds.feat_dim,
                                   ds.feat_dtype, xs)); // CombineMissData
    SAM_HIP(hipStreamSynchronize(xs));
    t_comb_miss = since(t0);
    t0 = clk::now();
    combine_hits();
    SAM_HIP(hipStreamSynchronize(xs));
    t_comb_hit = since(t0);
  } else {
    static const size_t chunk_mb = [] { const char *e = getenv("SAMGRAPH_STAGED_CHUNK_MB"); const long v = e ? atol(e) : 0; return (size_t)(v > 0 ? v : 16); }();
    static const size_t chunk_rows = [] { const char *e = getenv("SAMGRAPH_STAGED_CHUNK_ROWS"); const long v = e ? atol(e) : 0; return (size_t)(v > 0 ? v : 0); }(); // test hook
    const size_t chunk = chunk_rows ? chunk_rows : std::max<size_t>(1024, (chunk_mb << 20) / row_bytes);
    // ONE dispatch of the host team per batch: every thread walks the chunks itself (its slice of chunk 0, of chunk 1,
    // ...) and ticks the chunk's counter; the calling thread -- thread 0 of the team, the only one that talks to HIP --
    // hands every chunk whose counter is full to the copy engine between two of its own slices.  (One dispatch per
    // chunk was 34 wake-ups of 15 sleeping threads per batch: a millisecond of an 11-ms step.)
    const size_t nchunks = (num_miss + chunk - 1) / chunk;
    const int T = host_team_->size();
    std::vector<std::atomic<int>> ticks(nchunks);
    for (auto &t : ticks) t.store(0, std::memory_order_relaxed);
    size_t flushed = 0;
    auto flush_ready = [&](bool all) {
      while (flushed < nchunks) {
        if (ticks[flushed].load(std::memory_order_acquire) != T) {
          if (!all) return;
          std::this_thread::yield();
          continue;
        }
        const size_t lo = flushed * chunk, m = std::min(chunk, num_miss - lo);
        SAM_HIP(hipMemcpyAsync(land + lo * row_bytes, rows + lo * row_bytes, m * row_bytes, hipMemcpyHostToDevice, xs));
        if (have_cache)
          SAM_GGMS(ggms_gather_scatter(b->feat, (char *)b->miss_rows_dev + lo * row_bytes, nullptr, b->miss_dst + lo, m, nullptr,
                                       ds.feat_dim, ds.feat_dtype, xs)); // CombineMissData of this chunk
        ++flushed;
      }
    };
    t0 = clk::now();
    const char *feat = (const char *)ds.feat.ptr;
    const uint32_t *ids = b->miss_ids_host;
    const uint32_t mask = ds.feat_mask;
    host_team_->ParallelFor((size_t)T, [&](size_t tid, size_t, int) { // one iteration per thread: iteration == thread
      constexpr size_t kAhead = 8;
      for (size_t c = 0; c < nchunks; ++c) {
        const size_t base = c * chunk, m = std::min(chunk, num_miss - base);
        const size_t q = m / T, r = m % T;
        const size_t lo = base + tid * q + std::min<size_t>(tid, r), hi = lo + q + (tid < r ? 1 : 0);
        for (size_t i = lo; i < hi; ++i) {
          if (i + kAhead < hi) {
            const char *nx = feat + (size_t)(ids[i + kAhead] & mask) * row_bytes;
            for (size_t o = 0; o < row_bytes; o += 64) __builtin_prefetch(nx + o, 0, 0);
          }
          copy_row_stream(rows + i * row_bytes, feat + (size_t)(ids[i] & mask) * row_bytes, row_bytes);
        }
        store_fence();
        ticks[c].fetch_add(1, std::memory_order_release);
        if (tid == 0) flush_ready(false);
      }
    });
    t_gather = since(t0);
    flush_ready(true);
  }
  // the reference's step items (profiler.h:111-116: 44 .. 49); overlapped mode: the host's own busy time per phase
  prof.LogStep(b->key, 44, t_index);
  prof.LogStep(b->key, 45, t_ids);
  prof.LogStep(b->key, 46, t_gather);
  prof.LogStep(b->key, 47, t_copy);
  prof.LogStep(b->key, 48, t_comb_miss);
  prof.LogStep(b->key, 49, t_comb_hit);
  prof.LogEpochAdd(b->key, 20 /*extension: host gather seconds of the staged path*/, t_gather);
  prof.LogEpochAdd(b->key, 21 /*extension: H2D seconds (serial mode)*/, t_copy);
  prof.LogEpochAdd(b->key, 22 /*extension: combine-miss seconds (serial mode)*/, t_comb_miss);
  prof.LogEpochAdd(b->key, 23 /*extension: combine-cache seconds (serial mode)*/, t_comb_hit);
}

} // namespace sam
