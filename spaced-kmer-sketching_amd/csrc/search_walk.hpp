// The walk over reference batches that sks_search and sks_search_topk share
// (search_api.cpp, topk_api.cpp): the query set's join layout built once, the
// references taken in batches of whole 64-sketch blocks, each batch's layout
// built with the query layout's log_b and group bounds and joined with it into
// packed count tiles [b_blocks][q_blocks][64][64] (tile bj * q_blocks + qi, rows
// = queries), which the caller's kernel consumes before the next batch clears
// them; one wait at the end reads every layout's status words.
#pragma once
#include "sks_ctx.hpp"

namespace sks {

// packed count tiles of one reference batch (16 KB a tile): the default batch is
// the largest number of reference blocks whose tiles fit
constexpr uint64_t kSearchTileBudget = 256ull << 20;

// One call's walk.  plan() sizes the batches and carves c->lay: the group
// bounds, the query layout, one batch's layout, `head_words` words of the
// caller's followed by [1 + n_batches][2] status words (one span, cleared at the
// start and read back at the end), the (I, J) list of a full batch, its packed
// counts, the layout builds' temporary storage and `extra_bytes` of the
// caller's.  begin() queues everything up to the query layout, batch(b) one
// batch's layout and join, end() reads the span back (the one wait).
struct SearchWalk {
  // the plan
  uint32_t log_b = 0, G = 0, qb = 0, rb = 0, n_batches = 0, b_max_n = 0;
  uint64_t bb = 0, b_tot = 0, tiles_max = 0;
  int ew = 1;
  size_t head_words = 0, span_words = 0;
  Region<uint64_t> r_bounds;
  LayoutRegions r_q, r_b;
  Region<uint32_t> r_span, r_tiles;
  Region<int32_t> r_cnt;
  Region<char> r_tmp, r_extra;
  // after plan(): pointers into c->lay
  uint64_t* bounds = nullptr;
  LayoutArrays AQ{}, AB{};
  uint32_t* head = nullptr;  // the caller's words, then the status words
  uint32_t* stat = nullptr;  // the queries' status words; batch b's are stat + 2 * (1 + b)
  uint32_t* tiles = nullptr;
  int32_t* cnt = nullptr;
  void* tmp = nullptr;
  void* extra = nullptr;
  // after batch(b)
  uint32_t r0 = 0, rn = 0, nbb = 0;
  uint32_t* bstat = nullptr;
  // after end()
  std::vector<uint32_t> h_span;

  int plan(sks_ctx* c, const std::string& me, const SketchSpan& Q, const SketchSpan& R, int elem_words,
           size_t caller_head_words, size_t extra_bytes) {
    ew = elem_words;
    log_b = sks::join_log_b(std::max<uint32_t>(std::max(Q.max_size, R.max_size), 1));
    G = sks::join_layout_groups(log_b);
    qb = (Q.n + 63) / 64;
    rb = (R.n + 63) / 64;
    // reference blocks per batch: the caller's, else what the tile budget holds
    bb = c->search_batch ? c->search_batch : std::max<uint64_t>(1, kSearchTileBudget / ((uint64_t)qb * 16384));
    bb = std::min<uint64_t>(bb, rb);
    if ((uint64_t)qb * bb > 0x7fffffffull || (uint64_t)qb + rb > (1u << 25))
      return sks::fail(SKS_E_UNSUPPORTED, me + ": too many 64-sketch blocks for one batch");
    n_batches = (uint32_t)((rb + bb - 1) / bb);
    // the largest batch in elements (sizes its layout): one batch holds the whole
    // set, several are measured on the sizes themselves (read back when the
    // caller gave device arrays only)
    b_tot = R.total;
    if (n_batches > 1) {
      std::vector<uint32_t> own;
      const uint32_t* h_sizes = R.h_sizes;
      if (!h_sizes) {
        own.resize(R.n);
        SKS_HIP(sks::pinned_d2h(own.data(), R.sizes, (size_t)R.n * sizeof(uint32_t), c->stream));
        h_sizes = own.data();
      }
      b_tot = 0;
      for (uint64_t b0 = 0; b0 < R.n; b0 += bb * 64) {
        uint64_t t = 0;
        for (uint64_t i = b0; i < std::min<uint64_t>(R.n, b0 + bb * 64); ++i) t += h_sizes[i];
        b_tot = std::max(b_tot, t);
      }
    }
    tiles_max = (uint64_t)qb * bb;
    const size_t BW = sks::join_layout_boff_words(log_b);
    b_max_n = (uint32_t)std::min<uint64_t>(R.n, bb * 64);
    head_words = (caller_head_words + 1) & ~(size_t)1;  // the status words stay 8-byte aligned
    span_words = head_words + (size_t)(1 + n_batches) * 2;
    Carver cv;
    r_bounds = cv.take<uint64_t>((size_t)(G + 1) * ew);
    r_q = carve_layout(cv, Q.total, qb, BW, ew);
    r_b = carve_layout(cv, b_tot, (uint32_t)bb, BW, ew);
    r_span = cv.take<uint32_t>(span_words);
    r_tiles = cv.take<uint32_t>(tiles_max * 2);
    r_cnt = cv.take<int32_t>(tiles_max * 4096);
    r_tmp = cv.take<char>(std::max(sks::join_layout_temp_bytes(Q.n, log_b, ew),
                                   sks::join_layout_temp_bytes(b_max_n, log_b, ew)) + 256);
    r_extra = cv.take<char>(extra_bytes);
    SKS_HIP(c->lay.reserve(cv.need()));
    void* w = c->lay.ptr;
    bounds = r_bounds.in(w);
    AQ = r_q.in(w);
    AB = r_b.in(w);
    head = r_span.in(w);
    stat = head + head_words;
    tiles = r_tiles.in(w);
    cnt = r_cnt.in(w);
    tmp = r_tmp.in(w);
    extra = r_extra.in(w);
    return SKS_OK;
  }

  // h_bounds: the host group bounds to use ((G + 1) * ew words for log_b), or
  // null to sample them once from the references.
  int begin(sks_ctx* c, const SketchSpan& Q, const SketchSpan& R, const std::vector<uint64_t>* h_bounds) {
    SKS_HIP(hipEventRecord(c->ev_begin, c->stream));
    SKS_HIP(hipMemsetAsync(head, 0, span_words * 4, c->stream));
    // tile bj * qb + qi = (query block qi, batch block bj): queries are global
    // blocks [0, qb), the batch's blocks follow them, so I < J; a shorter last
    // batch joins a prefix of the same list
    {
      std::vector<uint32_t> h_tiles(tiles_max * 2);
      for (uint64_t bj = 0; bj < bb; ++bj)
        for (uint32_t qi = 0; qi < qb; ++qi) {
          h_tiles[2 * (bj * qb + qi)] = qi;
          h_tiles[2 * (bj * qb + qi) + 1] = qb + (uint32_t)bj;
        }
      SKS_HIP(sks::pinned_h2d(tiles, h_tiles.data(), h_tiles.size() * 4, c->stream));
    }
    SKS_TRY(queue_group_bounds(c, R, log_b, ew, h_bounds, bounds));
    // the query layout, once
    SKS_HIP(sks::join_layout_build(Q.data, Q.starts, Q.sizes, Q.n, log_b, ew, bounds, tmp, AQ.vals, AQ.masks, AQ.boff,
                                   AQ.bstart, stat, c->join_check, c->stream));
    return SKS_OK;
  }

  // batch b: references [r0, r0 + rn) in nbb blocks, their counts in cnt
  int batch(sks_ctx* c, const SketchSpan& R, uint32_t b) {
    r0 = (uint32_t)(b * bb * 64);
    rn = (uint32_t)std::min<uint64_t>(R.n - r0, bb * 64);
    nbb = (rn + 63) / 64;
    const uint64_t nt = (uint64_t)qb * nbb;
    bstat = stat + 2 * (1 + b);
    // the batch's layout with the query layout's log_b and bounds; its second
    // launch clears the batch's count tiles
    const sks::ZeroSpans zs{{reinterpret_cast<uint32_t*>(cnt), nullptr, nullptr}, {nt * 4096, 0, 0}};
    SKS_HIP(sks::join_layout_build(R.data, R.starts + r0, R.sizes + r0, rn, log_b, ew, bounds, tmp, AB.vals, AB.masks,
                                   AB.boff, AB.bstart, bstat, c->join_check, c->stream, &zs));
    // rows: the query layout (block 0 = global block 0); columns: the batch
    // (block 0 = global block qb); every cell of the (qb + nbb) * 64 square is
    // in range for the join, the consumer drops the padding rows and columns
    SKS_HIP(sks::join_launch(view_of(AQ), 0, view_of(AB), 0u - qb, (qb + nbb) * 64, log_b, ew, true, 0,
                             (qb + nbb) * 64, 0, nt, tiles, true, cnt, c->join_check, c->stream));
    return SKS_OK;
  }

  // The caller's words and every layout's status (one wait).  An invalid layout
  // records ev_end and fails with SKS_E_UNSUPPORTED: "<me>: the join layout of
  // ... could not be placed (invalid layout); <nothing>".
  int end(sks_ctx* c, const std::string& me, const char* nothing, bool* invalid_layout) {
    h_span.assign(span_words, 0);
    SKS_HIP(sks::pinned_d2h(h_span.data(), head, span_words * 4, c->stream));
    for (uint32_t b = 0; b <= n_batches; ++b)
      if (h_span[head_words + 2 * b + 1]) {
        SKS_HIP(hipEventRecord(c->ev_end, c->stream));
        return fail_invalid_layout(me, b ? "reference batch " + std::to_string(b - 1) : std::string("the queries"),
                                   nothing, invalid_layout);
      }
    return SKS_OK;
  }
};

}  // namespace sks
