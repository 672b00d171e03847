// list_heads.hip -- inline list heads: one 64-byte record per node of a static, unsharded CSR (include/ggms.h, "Inline
// list heads").  No reference counterpart.
//
// Why: a sampler input is a dependent chain -- indptr[v], indptr[v + 1] (one request), then the list at indices + b
// (one or two more lines, a few bytes used of each).  On papers100M an input emits 5.2 edges on average, so most lists
// are short: the record holds degree AND list for every node of degree <= 15, and an input costs one memory-side request
// and one round trip.  Longer lists keep their place in `indices`; their record carries degree and offset, which is what
// indptr gave.
//
//   k_list_heads_build   one streaming pass: a thread writes 16 bytes (a quarter of a record), so a wave writes 1 KiB
//                        contiguous; the 4 threads of a node read the same indptr pair (one line, served by the L1)
//   registry             host side, this process: handle id -> (heads, indptr, indices, num_node).  view_of()
//                        (ggms_device.h) asks it on every call that takes a graph whose heads_id is not 0; an id that is
//                        not live, or whose three values differ from the struct's, yields no heads
#include <mutex>

#include "ggms_internal.h"

namespace ggms {

namespace {

__global__ __launch_bounds__(kBlock) void k_list_heads_build(const uint32_t *__restrict__ indptr,
                                                             const uint32_t *__restrict__ indices, uint64_t num_node,
                                                             uint4 *__restrict__ heads) {
  const uint64_t quarters = 4 * num_node;
  for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < quarters; t += (uint64_t)gridDim.x * kBlock) {
    const uint64_t v = t >> 2;
    const uint32_t w0 = 4u * ((uint32_t)t & 3u); // my words: w0 .. w0 + 3 of the record
    uint32_t b, e;
    GraphView::bounds(indptr, (uint32_t)v, b, e);
    const uint32_t deg = e - b;
    uint32_t w[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t i = w0 + k;
      uint32_t x = 0;
      if (i == 0) x = deg;
      else if (deg <= kHeadInline) x = i <= deg ? indices[(uint64_t)b + i - 1] : 0u;
      else if (i == 1) x = b;
      w[k] = x;
    }
    heads[t] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

struct HeadsEntry {
  const void *heads;
  const uint32_t *indptr, *indices;
  uint32_t num_node;
  bool live;
};
std::mutex g_heads_mutex;
HeadsEntry g_heads[GGMS_LIST_HEADS_MAX + 1]; // [0] is never used: id 0 = none

void release_locked(uint32_t id) {
  if (id >= 1 && id <= GGMS_LIST_HEADS_MAX) g_heads[id] = HeadsEntry{};
}

} // namespace

const uint32_t *list_heads_of(const ggms_graph_t *g) {
  const uint32_t id = g->heads_id;
  if (id == 0 || id > GGMS_LIST_HEADS_MAX || g->num_part != 0) return nullptr;
  std::lock_guard<std::mutex> lock(g_heads_mutex);
  const HeadsEntry &h = g_heads[id];
  if (!h.live || h.indptr != g->indptr || h.indices != g->indices || h.num_node != g->num_node) return nullptr;
  return static_cast<const uint32_t *>(h.heads);
}

} // namespace ggms

using namespace ggms;

extern "C" {

size_t ggms_list_heads_bytes(size_t num_node) { return num_node * (size_t)GGMS_LIST_HEAD_BYTES; }

int ggms_list_heads_build(const ggms_graph_t *graph, void *heads, size_t bytes, ggms_stream_t stream) {
  GGMS_CHECK_ARG(graph);
  if (graph->num_part != 0) {
    set_error("ggms_list_heads_build: inline list heads are for unsharded graphs (num_part = %u)", graph->num_part);
    return GGMS_ERR_INVALID;
  }
  if (graph->num_node == 0) return GGMS_OK;
  GGMS_CHECK_ARG(graph->indptr && graph->indices && heads);
  GGMS_CHECK_ARG(((uintptr_t)heads & (GGMS_LIST_HEAD_BYTES - 1)) == 0);
  if (bytes < ggms_list_heads_bytes(graph->num_node)) {
    set_error("ggms_list_heads_build: %zu bytes for %u nodes, %zu needed", bytes, graph->num_node,
              ggms_list_heads_bytes(graph->num_node));
    return GGMS_ERR_INVALID;
  }
  hipLaunchKernelGGL(k_list_heads_build, dim3(grid_for(4 * (size_t)graph->num_node, kBlock)), dim3(kBlock), 0,
                     to_stream(stream), graph->indptr, graph->indices, (uint64_t)graph->num_node,
                     static_cast<uint4 *>(heads));
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

int ggms_list_heads_attach(ggms_graph_t *graph, const void *heads) {
  GGMS_CHECK_ARG(graph && heads);
  GGMS_CHECK_ARG(((uintptr_t)heads & (GGMS_LIST_HEAD_BYTES - 1)) == 0);
  if (graph->num_part != 0) {
    set_error("ggms_list_heads_attach: inline list heads are for unsharded graphs (num_part = %u)", graph->num_part);
    return GGMS_ERR_INVALID;
  }
  GGMS_CHECK_ARG(graph->indptr && graph->indices);
  std::lock_guard<std::mutex> lock(g_heads_mutex);
  // the struct's own handle goes first -- but only if it really is this CSR's (the word may be garbage)
  const uint32_t old = graph->heads_id;
  if (old >= 1 && old <= GGMS_LIST_HEADS_MAX && g_heads[old].live && g_heads[old].indptr == graph->indptr &&
      g_heads[old].indices == graph->indices && g_heads[old].num_node == graph->num_node)
    release_locked(old);
  graph->heads_id = 0;
  for (uint32_t id = 1; id <= GGMS_LIST_HEADS_MAX; ++id) {
    if (g_heads[id].live) continue;
    g_heads[id] = HeadsEntry{heads, graph->indptr, graph->indices, graph->num_node, true};
    graph->heads_id = id;
    return GGMS_OK;
  }
  set_error("ggms_list_heads_attach: all %d handles are in use", GGMS_LIST_HEADS_MAX);
  return GGMS_ERR_INVALID;
}

const void *ggms_list_heads_of(const ggms_graph_t *graph) { return graph ? list_heads_of(graph) : nullptr; }

int ggms_list_heads_detach(ggms_graph_t *graph) {
  GGMS_CHECK_ARG(graph);
  std::lock_guard<std::mutex> lock(g_heads_mutex);
  const uint32_t id = graph->heads_id;
  // as in attach: a handle is released only by a struct that matches it
  if (id >= 1 && id <= GGMS_LIST_HEADS_MAX && g_heads[id].live && g_heads[id].indptr == graph->indptr &&
      g_heads[id].indices == graph->indices && g_heads[id].num_node == graph->num_node)
    release_locked(id);
  graph->heads_id = 0;
  return GGMS_OK;
}

} // extern "C"
