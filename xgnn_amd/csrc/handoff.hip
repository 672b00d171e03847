// handoff.hip -- the batch hand-off of arch3 (one GPU samples, another trains): every array of one sampled batch
// copied from the sampler GPU's HBM to the trainer GPU's in ONE launch, with each array's length read on the device.
// The same kernel packs a batch into a slot of arch5's batch queue (host memory, on the sampler's device) and unpacks
// it on the trainer's device (ggms_queue_pack / ggms_queue_unpack, below).
//
// The reference copies a batch array by array (DoGraphCopy / DoIdCopy, cuda/cuda_loops.cc:600-655: Tensor::CopyTo per
// array, a StreamSync behind them), which needs every size on the host first.  Here the sizes stay where the sampler
// wrote them (the batch's counts words): a segment's length is read by the kernel, the grid is sized from the
// segment's upper bound, and the waves past the actual length exit at once.  The kernel runs on the trainer GPU and
// reads the sampler GPU's memory directly (a unified address over xGMI with peer access on; local HBM when both
// contexts name one device).
#include <cstddef>
#include <cstring>

#include <hip/hip_ext.h>

#include "ggms_internal.h"

namespace ggms {

typedef uint32_t u32x4_h __attribute__((ext_vector_type(4)));

constexpr int kHandoffUnroll = 4;                                 // 16-B chunks in flight per lane
constexpr uint64_t kHandoffBlockVecs = (uint64_t)kBlock * kHandoffUnroll; // 16-B chunks per workgroup (16 KiB)

// one segment as the kernel sees it: the host folds count_host and max_count into `bound`
struct HandoffSeg {
  const char *src;
  char *dst;
  const uint64_t *count_dev; // NULL: the length is `bound`
  uint64_t bound;            // elements: max_count, or min(count_host, max_count)
  uint32_t elem_bytes;
  uint32_t block_begin; // first workgroup of this segment; segment s owns [block_begin[s], block_begin[s + 1])
};
struct HandoffArgs {
  HandoffSeg seg[GGMS_HANDOFF_MAX_SEGS];
  uint32_t num_segs;
  uint32_t num_hdr;  // queue pack: header words written by the first lanes of workgroup 0
  uint64_t *hdr_dst;
  uint64_t hdr[3];
};

// Workgroup b copies 16 KiB of the segment it falls in: lane t moves chunks base + t + u * kBlock (u < 4), so every
// load instruction of a wave covers one contiguous KiB.  Bases are 16-B aligned (checked by the host), so the body
// needs no head; the < 16 tail bytes of a segment are copied byte by byte by the first lanes of its first workgroup.
__global__ __launch_bounds__(kBlock) void k_batch_handoff(HandoffArgs a) {
  const uint32_t b = blockIdx.x;
  uint32_t s = 0;
  while (s + 1 < a.num_segs && a.seg[s + 1].block_begin <= b) ++s; // wave-uniform: scalar loads of the kernel arguments
  const HandoffSeg &g = a.seg[s];
  uint64_t n = g.bound;
  if (g.count_dev) {
    const uint64_t c = *g.count_dev;
    n = c < n ? c : n; // never past the buffers the bound describes
  }
  const uint64_t bytes = n * g.elem_bytes, nvec = bytes >> 4;
  const uint64_t lb = b - g.block_begin;
  const uint32_t t = threadIdx.x;
  if (b == 0 && t < a.num_hdr) a.hdr_dst[t] = a.hdr[t];
  if (lb == 0 && t < (bytes & 15)) g.dst[(nvec << 4) + t] = g.src[(nvec << 4) + t];
  const uint64_t base = lb * kHandoffBlockVecs;
  if (base + (t & ~(uint32_t)(kWave - 1)) >= nvec) return; // this wave's first chunk is past the length
  const u32x4_h *src = reinterpret_cast<const u32x4_h *>(g.src);
  u32x4_h *dst = reinterpret_cast<u32x4_h *>(g.dst);
  if (base + kHandoffBlockVecs <= nvec) { // the whole workgroup's 16 KiB is inside the segment
    u32x4_h v[kHandoffUnroll];
#pragma unroll
    for (int u = 0; u < kHandoffUnroll; ++u) v[u] = __builtin_nontemporal_load(src + base + t + u * kBlock);
#pragma unroll
    for (int u = 0; u < kHandoffUnroll; ++u) __builtin_nontemporal_store(v[u], dst + base + t + u * kBlock);
    return;
  }
#pragma unroll
  for (int u = 0; u < kHandoffUnroll; ++u) {
    const uint64_t i = base + t + (uint64_t)u * kBlock;
    if (i < nvec) __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
  }
}

} // namespace ggms

using namespace ggms;

static int launch_segments(const ggms_copy_seg_t *segs, uint32_t num_segs, uint64_t *hdr_dst, const uint64_t *hdr,
                           uint32_t num_hdr, ggms_stream_t stream) {
  GGMS_CHECK_ARG(segs && num_segs >= 1 && num_segs <= GGMS_HANDOFF_MAX_SEGS && num_hdr <= 3);
  HandoffArgs a;
  std::memset(&a, 0, sizeof(a));
  a.num_segs = num_segs;
  a.num_hdr = num_hdr;
  a.hdr_dst = hdr_dst;
  for (uint32_t i = 0; i < num_hdr; ++i) a.hdr[i] = hdr[i];
  uint64_t blocks = 0;
  for (uint32_t s = 0; s < num_segs; ++s) {
    const ggms_copy_seg_t &in = segs[s];
    GGMS_CHECK_ARG(in.elem_bytes >= 1);
    GGMS_CHECK_ARG(in.max_count == 0 || (in.src && in.dst && (((uintptr_t)in.src | (uintptr_t)in.dst) & 15) == 0));
    HandoffSeg &g = a.seg[s];
    g.src = (const char *)in.src;
    g.dst = (char *)in.dst;
    g.count_dev = in.count_dev;
    g.bound = in.count_dev ? in.max_count : (in.count_host < in.max_count ? in.count_host : in.max_count);
    g.elem_bytes = in.elem_bytes;
    g.block_begin = (uint32_t)blocks;
    const uint64_t vecs = (g.bound * in.elem_bytes) >> 4; // the body's 16-B chunks at the bound
    const uint64_t nb = vecs ? (vecs + kHandoffBlockVecs - 1) / kHandoffBlockVecs : 1; // >= 1: the tail's workgroup
    blocks += nb;
    GGMS_CHECK_ARG(blocks < (1ull << 31));
  }
  hipStream_t st = to_stream(stream);
  hipEvent_t t0 = nullptr, t1 = nullptr;
  if (take_armed_timer(&t0, &t1)) // a launch timer armed on this thread rides on the dispatch packet
    hipExtLaunchKernelGGL(k_batch_handoff, dim3((uint32_t)blocks), dim3(kBlock), 0, st, t0, t1, 0, a);
  else
    hipLaunchKernelGGL(k_batch_handoff, dim3((uint32_t)blocks), dim3(kBlock), 0, st, a);
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

static uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

// the slot's segments, batch side <-> slot side, in one order for both directions: per layer row, col (, data), then
// input nodes, output nodes, counts words.  `to_slot`: pack (lengths from the batch's counts words), else unpack
// (lengths from the slot's header).
static int queue_segments(ggms_copy_seg_t *segs, uint32_t *n, const ggms_queue_layout_t *lay, const ggms_queue_batch_t *b,
                          char *slot, uint64_t num_output, bool to_slot) {
  const uint32_t L = lay->num_layer;
  ggms_queue_header_t *h = reinterpret_cast<ggms_queue_header_t *>(slot);
  const uint64_t *counts = to_slot ? b->counts : h->counts; // where the kernel reads the lengths
  uint32_t k = 0;
  auto add = [&](void *batch_side, uint64_t off, const uint64_t *count_dev, uint64_t count_host, uint64_t max_count,
                 uint32_t elem_bytes) {
    void *slot_side = slot + off;
    segs[k++] = ggms_copy_seg_t{to_slot ? batch_side : slot_side, to_slot ? slot_side : batch_side, count_dev, count_host,
                                max_count, elem_bytes, 0};
  };
  for (uint32_t i = 0; i < L; ++i) {
    if (!b->row[i] || !b->col[i] || (lay->has_data && !b->data[i])) return GGMS_ERR_INVALID;
    add(b->row[i], lay->off_row[i], counts + GGMS_COUNT_EDGES(i), 0, lay->max_edges[i], 4);
    add(b->col[i], lay->off_col[i], counts + GGMS_COUNT_EDGES(i), 0, lay->max_edges[i], 4);
    if (lay->has_data) add(b->data[i], lay->off_data[i], counts + GGMS_COUNT_EDGES(i), 0, lay->max_edges[i], 4);
  }
  if (!b->input_nodes || !b->output_nodes || !b->counts) return GGMS_ERR_INVALID;
  add(b->input_nodes, lay->off_input, counts + GGMS_COUNT_INPUT(L), 0, lay->max_input, 4);
  if (to_slot) add(b->output_nodes, lay->off_output, nullptr, num_output, lay->max_output, 4);
  else add(b->output_nodes, lay->off_output, &h->num_output, 0, lay->max_output, 4);
  add(b->counts, offsetof(ggms_queue_header_t, counts), nullptr, GGMS_COUNTS_WORDS(L), GGMS_COUNTS_WORDS(L), 8);
  *n = k;
  return GGMS_OK;
}

extern "C" {

int ggms_batch_handoff(const ggms_copy_seg_t *segs, uint32_t num_segs, ggms_stream_t stream) {
  return launch_segments(segs, num_segs, nullptr, nullptr, 0, stream);
}

int ggms_queue_layout(ggms_queue_layout_t *lay, uint32_t num_layer, const size_t *max_edges, size_t max_input,
                      size_t max_output, int has_data) {
  GGMS_CHECK_ARG(lay && max_edges && num_layer >= 1 && num_layer <= GGMS_QUEUE_MAX_LAYERS);
  static_assert(sizeof(ggms_queue_header_t) == 512, "the slot header is 512 bytes");
  std::memset(lay, 0, sizeof(*lay));
  lay->num_layer = num_layer;
  lay->has_data = has_data ? 1 : 0;
  lay->max_input = max_input;
  lay->max_output = max_output;
  uint64_t off = sizeof(ggms_queue_header_t);
  auto place = [&](uint64_t elems) { const uint64_t at = off; off = align_up(off + elems * 4, 256); return at; };
  for (uint32_t i = 0; i < num_layer; ++i) {
    lay->max_edges[i] = max_edges[i];
    lay->off_row[i] = place(max_edges[i]);
    lay->off_col[i] = place(max_edges[i]);
    if (has_data) lay->off_data[i] = place(max_edges[i]);
  }
  lay->off_input = place(max_input);
  lay->off_output = place(max_output);
  lay->slot_bytes = align_up(off, 4096);
  return GGMS_OK;
}

int ggms_queue_pack(void *slot, const ggms_queue_layout_t *lay, const ggms_queue_batch_t *src, uint64_t key,
                    uint64_t num_output, ggms_stream_t stream) {
  GGMS_CHECK_ARG(slot && lay && src && ((uintptr_t)slot & 15) == 0);
  GGMS_CHECK_ARG(lay->num_layer >= 1 && lay->num_layer <= GGMS_QUEUE_MAX_LAYERS && lay->slot_bytes > 0);
  ggms_copy_seg_t segs[GGMS_HANDOFF_MAX_SEGS];
  uint32_t n = 0;
  GGMS_CHECK_ARG(queue_segments(segs, &n, lay, src, (char *)slot, num_output, true) == GGMS_OK);
  ggms_queue_header_t *h = reinterpret_cast<ggms_queue_header_t *>(slot);
  const uint64_t hdr[3] = {key, num_output < lay->max_output ? num_output : lay->max_output, lay->num_layer};
  return launch_segments(segs, n, &h->key, hdr, 3, stream); // key, num_output, num_layer: consecutive words
}

int ggms_queue_unpack(const ggms_queue_batch_t *dst, const void *slot, const ggms_queue_layout_t *lay,
                      ggms_stream_t stream) {
  GGMS_CHECK_ARG(slot && lay && dst && ((uintptr_t)slot & 15) == 0);
  GGMS_CHECK_ARG(lay->num_layer >= 1 && lay->num_layer <= GGMS_QUEUE_MAX_LAYERS && lay->slot_bytes > 0);
  ggms_copy_seg_t segs[GGMS_HANDOFF_MAX_SEGS];
  uint32_t n = 0;
  GGMS_CHECK_ARG(queue_segments(segs, &n, lay, dst, (char *)slot, 0, false) == GGMS_OK);
  return launch_segments(segs, n, nullptr, nullptr, 0, stream);
}

} // extern "C"
