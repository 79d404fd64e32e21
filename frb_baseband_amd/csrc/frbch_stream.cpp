// libfrbch: stream state of a handle -- batches, the rescale-interval state machine (buffered and two-pass forms), the chain of
// stages of a scan and the two kernels that may share the chip (frbch_internal.h lists the units).
#include "frbch_internal.h"

namespace frbchi {

// Close the rescale interval that sits at the front of powbuf: statistics over `stat_rows` rows,
// then digitise `emit_rows` rows into dst and keep the rest for the next interval.
struct Chain;
int chain_quant_lane_cus(const Chain* c);
dev_stream_t chain_quant_stream(Chain* c, dev_stream_t s, int* ncu);
void chain_quant_done(Chain* c, dev_stream_t sq);
int finalize_interval(frbch_handle* h, uint64_t stat_rows, uint8_t* d_out, size_t cap, uint64_t* rows_written,
                      dev_stream_t s0, Chain* ch = nullptr) {
  const Plan& pl = h->pl;
  if (h->quant_busy) {   // a digitiser of the previous interval (and its move of the remaining rows) still works on the power buffer
    (void)dev_stream_wait(s0, h->quant_ev);
    h->quant_busy = false;
  }
  int rc = run_stats(h, stat_rows, s0);
  if (rc) return rc;
  // the scan's second stream when the digitiser can run beside the next K1 (on CUs it holds by an LDS reservation: only the lean
  // kernel does that)
  dev_stream_t s = s0;
  {
    const int lane = chain_quant_lane_cus(ch);
    uint64_t a_ = 0, b_ = 0, c_ = 0;
    if (lane && quant_fast_geometry(h, lane, &a_, &b_, &c_)) s = chain_quant_stream(ch, s0, &h->quant_lane_cus);
  }
  h->have_scale = true;
  if (h->cfg.rescale_constant) h->scale_frozen = true;
  const uint64_t emit_rows = h->scale_frozen ? h->pow_rows : stat_rows;
  if (out_extent(h, *rows_written + emit_rows) > cap)
    return fail(h, FRBCH_E_CAPACITY, "output buffer too small for the rows of a completed rescale interval");
  rc = run_quantise(h, emit_rows, d_out + *rows_written * out_row_span(h), s, s != s0 ? h->quant_lane_cus : 0);
  if (rc) return rc;
  *rows_written += emit_rows;
  h->rows_out += emit_rows;
  const uint64_t rest = h->pow_rows - emit_rows;
  // forward chunked move (chunks no longer than the shift distance never overlap)
  uint64_t done = 0;
  while (done < rest) {
    const uint64_t len = std::min<uint64_t>(emit_rows, rest - done);
    CHECK_DEV(h, dev_d2d(h->powbuf + done * pl.ncol, h->powbuf + (emit_rows + done) * pl.ncol,
                         len * pl.ncol * sizeof(float), s), "move power rows");
    done += len;
  }
  h->pow_rows = rest;
  h->fused_rows = 0;
  h->fused_valid = false;   // (re-armed when an interval starts on an empty buffer)
  if (s != s0) {            // later work of this handle on the power buffer / the codes is ordered behind the digitiser
    if (!h->quant_ev_made) { (void)dev_event_create_sync(&h->quant_ev); h->quant_ev_made = true; }
    dev_event_record(h->quant_ev, s);
    h->quant_busy = true;
    chain_quant_done(ch, s);
  }
  return FRBCH_OK;
}

bool fused_ok(const frbch_handle* h) { return h->scale_frozen; }

// ---- two-pass rescale of a first interval (`-c`, which the reference always passes, process_vdif.py:157,160) -------------------
// The buffered form writes the float rows of the interval (8 B per dual-pol sample with four products), reads them back in the
// digitiser and moves 26 B per sample behind K1; with frbch_k2_priv the batch's spill is still resident when the interval is
// complete, so K2 runs over it twice instead: a statistics-only pass (sums, no rows), frbch_stats_final, then the digitising pass --
// 18 B per sample, and the SAME float arithmetic in both passes, so the codes are what the buffered form produces from the same
// offset / scale.  Taken when the interval starts with this batch and either ends inside it or the batch is the last of the call
// (the flush, or the next call, then finds the batch deferred).  Automatic for four products (measured, config 3: 35.3 ms per 8-IF
// step against 36.0 buffered); one product stays buffered (its float rows are a quarter of the bytes: 3.3
// against 3.9 ms at config 2).  flags: 1 << 27 forces the buffered form, 1 << 28 the two-pass form.
bool twopass_usable(const frbch_handle* h) {
  const Plan& pl = h->pl;
  if (!(pl.fast_k2_priv && h->priv_grid > 0 && h->cfg.rescale_constant && pl.interval_rows > 0 && !pl.k2_two_stage && fused_chunks_of(h) > 0))
    return false;
  if (h->cfg.flags & kFlagBuffered) return false;
  return (h->cfg.flags & kFlagTwoPass) || pl.nif == 4;
}
// second pass over a deferred batch: offset / scale are final, K2 digitises the batch's rows into d_out
int deferred_emit(frbch_handle* h, uint8_t* d_out, size_t cap, uint64_t* rows_written, dev_stream_t s) {
  frbch_handle::Deferred& d = h->deferred;
  if (out_extent(h, *rows_written + d.rows) > cap) return fail(h, FRBCH_E_CAPACITY, "output buffer too small for the rows of a completed rescale interval");
  KParams p = d.p;
  p.offset = h->offset;
  p.scale = h->scale;
  p.out_mode = FRBCH_OUT_CODES;
  p.code_out = d_out;
  p.row0 = *rows_written;
  p.out_pitch = h->out_pitch ? h->out_pitch : (uint64_t)h->pl.c;
  p.stat_partial = nullptr;
  const int rc = launch_back(h, p, d.nb, s);
  if (rc) return rc;
  *rows_written += d.rows;
  h->rows_out += d.rows;
  d.active = false;
  return FRBCH_OK;
}
// more blocks arrive while a batch is deferred and its interval is still open: the batch becomes the front of the buffered
// interval after all (one K2 pass writes its float rows; its sums are already in the partial table)
int deferred_materialise(frbch_handle* h, dev_stream_t s) {
  frbch_handle::Deferred& d = h->deferred;
  int rc = ensure_powbuf(h);
  if (rc) return rc;
  if (d.rows > h->pow_cap_rows) return fail(h, FRBCH_E_STATE, "power buffer overflow");
  KParams p = d.p;
  p.out_mode = FRBCH_OUT_FLOAT_POWER;
  p.power_out = h->powbuf;
  p.row0 = 0;
  p.stat_partial = nullptr;
  rc = launch_back(h, p, d.nb, s);
  if (rc) return rc;
  h->pow_rows = d.rows;
  d.active = false;
  return FRBCH_OK;
}

std::mutex g_lanes_mutex;
std::vector<std::pair<std::pair<int, int>, Lanes*>> g_lanes;   // (device, CUs left to K1) -> lanes; live until the process ends

Lanes* get_lanes(int device, int ncu_front) {
  std::lock_guard<std::mutex> lk(g_lanes_mutex);
  for (auto& e : g_lanes)
    if (e.first.first == device && e.first.second == ncu_front) return e.second->ok ? e.second : nullptr;
  Lanes* ln = new Lanes();
  g_lanes.push_back({{device, ncu_front}, ln});
  ln->ncu = dev_cu_count(device);
  // a plain stream (no CU mask: a masked queue costs every launch of the process 50 - 100 us while it is active,
  // profiles/NOTES.md); the digitiser claims its CUs by its LDS reservation, ncu_f is what is left for the K1 beside it.
  // (a failed creation leaves the entry with ok = false: later calls get nullptr)
  if (ln->ncu <= 0 || ncu_front < 8 || ncu_front > ln->ncu - 8) return nullptr;
  if (dev_stream_create(&ln->b) != 0) {
    ln->b = 0;
    (void)dev_last_error_string();
    return nullptr;
  }
  ln->ncu_f = ncu_front;
  ln->ok = true;
  return ln;
}

dev_event_t pool_event(frbch_handle* h) {
  if (h->evpool.empty()) {
    h->evpool.resize(64);
    for (auto& e : h->evpool) (void)dev_event_create_sync(&e);
  }
  const dev_event_t e = h->evpool[h->evnext];
  h->evnext = (h->evnext + 1) % h->evpool.size();
  return e;
}


void chain_begin(Chain* c, frbch_handle* owner, dev_stream_t user, Lanes* ln, uint32_t stages_total) {
  *c = Chain();
  c->owner = owner;
  c->user = user;
  c->ln = stages_total >= 2 ? ln : nullptr;
  c->stages_total = stages_total;
  if (c->ln) {
    c->ev_entry = pool_event(owner);
    dev_event_record(c->ev_entry, user);
  }
}
// a front stage is queued on the caller's stream: the CUs left to its K1 when it shares the chip with the digitiser the back
// stage before it sent to the second stream, else 0 (all of them)
int chain_front(Chain* c) {
  const bool beside = c->ln && c->q_pending;
  c->q_pending = false;
  c->fronts++;
  return beside ? c->ln->ncu_f : 0;
}
// CUs the digitiser of a completed interval would hold on the second stream, negative: held by its LDS reservation (see
// run_quantise); 0 = no second stream, or no front stage left to run beside it
int chain_quant_lane_cus(const Chain* c) {
  if (!c || !c->ln || c->fronts >= c->stages_total) return 0;
  return -(c->ln->ncu - c->ln->ncu_f);
}
// the second stream for that digitiser, ordered behind the statistics in front of it on `s`
dev_stream_t chain_quant_stream(Chain* c, dev_stream_t s, int* ncu) {
  if (!chain_quant_lane_cus(c)) return s;
  const dev_stream_t sq = c->ln->b;
  *ncu = chain_quant_lane_cus(c);
  if (!c->b_rooted) {   // (implied by the wait on `e` below, recorded later on the same stream: kept as the lane's explicit root)
    (void)dev_stream_wait(sq, c->ev_entry);
    c->b_rooted = true;
  }
  const dev_event_t e = pool_event(c->owner);
  dev_event_record(e, s);               // behind the statistics
  (void)dev_stream_wait(sq, e);
  return sq;
}
void chain_quant_done(Chain* c, dev_stream_t sq) {
  if (!c || !c->ln || sq != c->ln->b) return;
  c->ev_q = pool_event(c->owner);
  dev_event_record(c->ev_q, sq);
  c->q_pending = true;
  c->have_q = true;
}
// everything the chain queued is ordered in front of what follows on the caller's stream
void chain_end(Chain* c) {
  if (c->ln && c->have_q) (void)dev_stream_wait(c->user, c->ev_q);
}

// front CUs requested through frbch_config::overlap (0 = automatic)
int overlap_front_cus(const frbch_handle* h) {
  const uint32_t v = h->cfg.overlap & 0xFFFFu;
  if (v == 1) return 0;                       // overlap off
  if (v) return (int)(v / 8 * 8);
  // automatic.  K1 beside K2: never -- both scale with their share of the CUs (K2 on 96 CUs takes 2.4x its whole-chip time),
  // splitting the chip between them only adds launches (profiles/r03_overlap_sweep_*.txt).
  // The digitiser of a completed interval beside the next IF's K1 (a scan): yes when it is a stream of four products
  // -- 6.4 GB per IF, HBM-bound on the whole chip with most CUs idle, while K1 is bound by its waves and leaves HBM half idle.
  // 80 of 256 CUs for the digitiser make both take ~2.3 ms (1.55 + 1.14 one after the other): 39.5 -> 36.4 ms per 8-IF step of
  // config 3, the two together moving 5.2 TB/s.  One product (1.6 GB): what it hides is what K1 loses on fewer CUs: off.
  const Plan& pl = h->pl;
  if (pl.nif == 4 && h->cfg.nbit_out == 8 && k1_paired_planned(pl) && h->lane_ncu >= 64)
    return h->lane_ncu * 11 / 16 / 8 * 8;
  return 0;
}
bool overlap_usable(const frbch_handle* h) {
  const Plan& pl = h->pl;
  return !pl.coherent && pl.fast_k1_log2m && pl.fast_k1_wave && k2_wave_planned(pl) &&
         overlap_front_cus(h) >= 8;
}

// Transform `nblocks` blocks starting `payload_off` bytes into the payload stream of d_frames.
int engine_feed_run(frbch_handle* h, const uint8_t* d_frames, uint32_t frame_bytes, uint32_t header_bytes,
                    uint64_t payload_off, uint64_t nblocks, uint8_t* d_out, size_t cap, uint64_t* rows_written,
                    dev_stream_t s, const uint32_t* d_fbad, Chain* chain);

// `h_bad` (optional): one flag per frame of d_frames, 1 = the frame is flagged invalid or is a filler for a missing frame
// number; `d_fbad` the same as a bitmap on the device.  Blocks that touch such a frame go through the generic K1, which
// reads their samples as 0; all other blocks take the fast kernels as before.
// `chain` (optional): the caller's chain of stages (a scan queues several IFs into one); else the call runs its own.
int engine_feed(frbch_handle* h, const uint8_t* d_frames, uint32_t frame_bytes, uint32_t header_bytes,
                uint64_t payload_off, uint64_t nblocks, uint8_t* d_out, size_t cap, uint64_t* rows_written,
                dev_stream_t s, const uint8_t* h_bad, uint64_t nfr_bad, const uint32_t* d_fbad, Chain* chain) {
  const Plan& pl = h->pl;
  *rows_written = 0;
  bool any = false;
  for (uint64_t f = 0; h_bad && f < nfr_bad && !any; ++f) any = h_bad[f] != 0;
  if (!any) return engine_feed_run(h, d_frames, frame_bytes, header_bytes, payload_off, nblocks, d_out, cap, rows_written, s, nullptr, chain);
  const uint64_t pb = frame_bytes - header_bytes;
  auto dirty = [&](uint64_t b) {
    const uint64_t a0 = payload_off + b * pl.block_stride_bytes, a1 = a0 + pl.block_payload_bytes - 1;
    for (uint64_t f = a0 / pb; f <= a1 / pb && f < nfr_bad; ++f)
      if (h_bad[f]) return true;
    return false;
  };
  for (uint64_t b0 = 0; b0 < nblocks;) {
    const bool d0 = dirty(b0);
    uint64_t b1 = b0 + 1;
    while (b1 < nblocks && dirty(b1) == d0) ++b1;
    const int rc = engine_feed_run(h, d_frames, frame_bytes, header_bytes, payload_off + b0 * pl.block_stride_bytes, b1 - b0, d_out, cap,
                                   rows_written, s, d0 ? d_fbad : nullptr, nullptr);
    if (rc) return rc;
    b0 = b1;
  }
  return FRBCH_OK;
}

// batches a run of `nblocks` blocks is cut into: equal sizes (no short tail launch), at most maxb blocks each
static void plan_batches(const Plan& pl, uint64_t nblocks, uint64_t* nbatch, uint64_t* per) {
  const uint64_t cap = pl.maxb;
  uint64_t nb = (nblocks + cap - 1) / cap;
  nb = std::max<uint64_t>(1, std::min<uint64_t>(nb, nblocks));
  *nbatch = nb;
  *per = nblocks ? (nblocks + nb - 1) / nb : 0;
  if (*per) *nbatch = (nblocks + *per - 1) / *per;
}
uint64_t feed_stage_count(const frbch_handle* h, uint64_t nblocks) {
  uint64_t nbatch = 0, per = 0;
  plan_batches(h->pl, nblocks, &nbatch, &per);
  return nblocks ? nbatch : 0;
}

// one run of blocks; *rows_written is the running row count of the call (rows land behind those already written).  Every stage
// goes to `s`; on a scan's chain the digitiser of a completed interval may go to the chain's second stream beside the next K1.
int engine_feed_run(frbch_handle* h, const uint8_t* d_frames, uint32_t frame_bytes, uint32_t header_bytes,
                    uint64_t payload_off, uint64_t nblocks, uint8_t* d_out, size_t cap, uint64_t* rows_written,
                    dev_stream_t s, const uint32_t* d_fbad, Chain* chain) {
  const Plan& pl = h->pl;
  if (!nblocks) return FRBCH_OK;
  uint64_t nbatch = 0, per = 0;
  plan_batches(pl, nblocks, &nbatch, &per);
  if (!h->spill_ev_made) {
    (void)dev_event_create_sync(&h->spill_ev);
    h->spill_ev_made = true;
  }
  int rc = FRBCH_OK;
  // a batch deferred by the two-pass rescale whose interval goes on: its float rows are written NOW, before the front stage of
  // the next batch overwrites the spill they come from
  if (h->deferred.active && !fused_ok(h)) rc = deferred_materialise(h, s);
  for (uint64_t b0 = 0; b0 < nblocks && !rc; b0 += per) {
    const uint32_t nb = (uint32_t)std::min<uint64_t>(per, nblocks - b0);
    KParams p = base_params(h);
    p.fbad = d_fbad;
    p.fbad_frame0 = 0;
    p.frames = d_frames;
    p.frame_bytes = frame_bytes;
    p.header_bytes = header_bytes;
    p.payload_bytes = frame_bytes - header_bytes;
    p.payload_off = payload_off + b0 * pl.block_stride_bytes;
    // ---- front: K0, K1, Kc --------------------------------------------------------------------------------------
    // on a scan's chain the back stage that read the spill last (maybe on the stream of an earlier call) must be through
    if (h->spill_busy && chain) (void)dev_stream_wait(s, h->spill_ev);
    h->spill_busy = false;
    h->lane_cus = chain ? chain_front(chain) : 0;
    rc = launch_front(h, p, nb, s);
    h->lane_cus = 0;
    if (rc) break;
    // ---- back: K2 (+ statistics and digitiser of a completed interval) ------------------------------------------
    if (h->quant_busy) {   // a digitiser of this handle on the scan's second stream still reads the power buffer
      (void)dev_stream_wait(s, h->quant_ev);
      h->quant_busy = false;
    }
    const uint64_t rows = (uint64_t)nb * pl.rows_per_block;
    if (fused_ok(h)) {
      if (out_extent(h, *rows_written + rows) > cap) { rc = fail(h, FRBCH_E_CAPACITY, "output buffer too small"); break; }
      p.out_mode = FRBCH_OUT_CODES;
      p.code_out = d_out;
      p.row0 = *rows_written;
      rc = launch_back(h, p, nb, s);
      if (rc) break;
      *rows_written += rows;
      h->rows_out += rows;
    } else if (!h->deferred.active && h->pow_rows == 0 && twopass_usable(h) && p.tile_major == 2 &&
               (rows >= pl.interval_rows || b0 + per >= nblocks)) {
      // ---- two-pass rescale: statistics-only pass now, the digitising pass once the interval is complete ----------------------
      rc = ensure_partial(h);
      if (rc) break;
      p.out_mode = FRBCH_OUT_STATS;
      p.row0 = 0;
      p.stat_partial = h->partial;
      p.stat_limit = pl.interval_rows;
      rc = clear_partial(h, p, nb, s);   // (frbch_k2_priv: nothing to clear)
      if (rc) break;
      rc = launch_back(h, p, nb, s);
      if (rc) break;
      h->fused_rows = std::min<uint64_t>(rows, pl.interval_rows);
      h->fused_valid = true;
      h->deferred.active = true;
      h->deferred.p = p;
      h->deferred.p.stat_first = 0;   // (the batch's later passes start no interval)
      h->deferred.nb = nb;
      h->deferred.rows = rows;
      if (rows >= pl.interval_rows) {   // the interval ends inside this batch: offset / scale now, then every row of the batch
        rc = run_stats(h, pl.interval_rows, s);
        if (rc) break;
        h->have_scale = true;
        h->scale_frozen = true;        // (-c: twopass_usable)
        h->fused_rows = 0;
        h->fused_valid = false;
        rc = deferred_emit(h, d_out, cap, rows_written, s);
        if (rc) break;
      }
    } else {
      rc = ensure_powbuf(h);
      if (rc) break;
      if (h->pow_rows + rows > h->pow_cap_rows) { rc = fail(h, FRBCH_E_STATE, "power buffer overflow"); break; }
      p.out_mode = FRBCH_OUT_FLOAT_POWER;
      p.power_out = h->powbuf;
      p.row0 = h->pow_rows;
      const bool starts = h->pow_rows == 0 && h->fused_chunks;   // an interval starts here: K2 can sum it while writing it
      if (starts) {
        h->fused_rows = 0;
        h->fused_valid = true;
      }
      if (h->fused_valid) {
        p.stat_partial = h->partial;
        p.stat_limit = pl.interval_rows;
      }
      if (starts) rc = clear_partial(h, p, nb, s);
      else if (p.stat_partial) rc = extend_partial(h, s);   // (the interval goes on: whichever K2 takes this launch finds its rows cleared)
      if (rc) break;
      rc = launch_back(h, p, nb, s);
      if (rc) break;
      if (h->fused_valid) {
        if (p.stat_partial) {
          const uint64_t room = pl.interval_rows > h->pow_rows ? pl.interval_rows - h->pow_rows : 0;
          h->fused_rows += std::min<uint64_t>(rows, room);
        } else {
          h->fused_valid = false;   // this launch ran a kernel that does not accumulate
        }
      }
      h->pow_rows += rows;
      while (!rc && !fused_ok(h) && h->pow_rows >= pl.interval_rows) rc = finalize_interval(h, pl.interval_rows, d_out, cap, rows_written, s, chain);
      if (rc) break;
    }
    if (chain) {
      dev_event_record(h->spill_ev, s);
      h->spill_busy = true;
    }
    h->blocks_done += nb;
  }
  return rc;
}

int engine_flush(frbch_handle* h, uint8_t* d_out, size_t cap, uint64_t* rows_written, dev_stream_t s, Chain* ch) {
  *rows_written = 0;
  if (h->deferred.active && !fused_ok(h)) {   // the scan ended inside its first interval: statistics over what there is, then the digitising pass
    int rc = run_stats(h, h->deferred.rows, s);
    if (rc) return rc;
    h->have_scale = true;
    if (h->cfg.rescale_constant) h->scale_frozen = true;
    h->fused_rows = 0;
    h->fused_valid = false;
    return deferred_emit(h, d_out, cap, rows_written, s);
  }
  if (fused_ok(h) || h->pow_rows == 0) return FRBCH_OK;
  if (h->quant_busy) {
    (void)dev_stream_wait(s, h->quant_ev);
    h->quant_busy = false;
  }
  return finalize_interval(h, std::min<uint64_t>(h->pow_rows, h->pl.interval_rows), d_out, cap, rows_written, s, ch);
}

// offset = 0, scale = 1 on the handle's stream.  Not waited for: work that follows on ANOTHER stream is ordered behind an event
// (join_reset); a reset of the 8 handles of a scan used to cost 8 host round trips with the GPU idle.
int set_identity_rescale(frbch_handle* h) {
  const Plan& pl = h->pl;
  CHECK_DEV(h, dev_memset32(h->offset, 0u, pl.ncol, h->stream), "clear offset");
  CHECK_DEV(h, dev_memset32(h->scale, 0x3F800000u, pl.ncol, h->stream), "unit scale");     // 1.0f
  if (!h->reset_ev_made) {
    CHECK_DEV(h, dev_event_create_sync(&h->reset_ev), "hipEventCreate");
    h->reset_ev_made = true;
  }
  dev_event_record(h->reset_ev, h->stream);
  h->reset_pending = true;
  return FRBCH_OK;
}
// the device entry points: stream `s` continues behind the handle's pending reset
void join_reset(frbch_handle* h, dev_stream_t s) {
  if (!h->reset_pending) return;
  if (s != h->stream) (void)dev_stream_wait(s, h->reset_ev);
  h->reset_pending = false;
}


}  // namespace frbchi
