// fragment_stream.cpp -- see fragment_stream.h
#include "fragment_stream.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <stdexcept>

#include "device_api.h"
#if defined(BROTLI_HOST_EMU)
#include "fragment_seam_emu.inc"  // the host emulation of frag_compress_jobs / frag_join_bounded
#endif

namespace brotli_mi355x {

namespace {

// InitCommandPrefixCodes, encode.rs:627-659
void InitCommandPrefixCodes(FragmentState* st) {
  static const uint8_t kDefaultCommandDepths[128] = {
      0,  4,  4,  5,  6,  6,  7,  7,  7,  7,  7,  8,  8,  8,  8,  8,  0,  0,  0,  4,  4,  4,  4,  4,  5,  5,
      6,  6,  6,  6,  7,  7,  7,  7,  10, 10, 10, 10, 10, 10, 0,  4,  4,  5,  5,  5,  6,  6,  7,  8,  8,  9,
      10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 5,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,
      0,  0,  6,  6,  6,  6,  6,  6,  5,  5,  5,  5,  5,  5,  4,  4,  4,  4,  4,  4,  4,  5,  5,  5,  5,  5,
      5,  6,  6,  7,  7,  7,  8,  10, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 0,  0,  0,  0};
  static const uint16_t kDefaultCommandBits[128] = {
      0,   0,   8,   9,   3,    35,   7,    71,   39,   103,  23,   47,   175,  111,  239,  31,   0,  0,  0,  4,
      12,  2,   10,  6,   13,   29,   11,   43,   27,   59,   87,   55,   15,   79,   319,  831,  191, 703, 447, 959,
      0,   14,  1,   25,  5,    21,   19,   51,   119,  159,  95,   223,  479,  991,  63,   575,  127, 639, 383, 895,
      255, 767, 511, 1023, 14,  0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,   0,   0,   0,
      27,  59,  7,   39,  23,   55,   30,   1,    17,   9,    25,   5,    0,    8,    4,    12,   2,   10,  6,   21,
      13,  29,  3,   19,  11,   15,   47,   31,   95,   63,   127,  255,  767,  2815, 1791, 3839, 511, 2559, 1535, 3583,
      1023, 3071, 2047, 4095, 0, 0,   0,    0};
  static const uint8_t kDefaultCommandCode[57] = {
      0xff, 0x77, 0xd5, 0xbf, 0xe7, 0xde, 0xea, 0x9e, 0x51, 0x5d, 0xde, 0xc6, 0x70, 0x57, 0xbc, 0x58, 0x58, 0x58, 0xd8,
      0xd8, 0x58, 0xd5, 0xcb, 0x8c, 0xea, 0xe0, 0xc3, 0x87, 0x1f, 0x83, 0xc1, 0x60, 0x1c, 0x67, 0xb2, 0xaa, 0x06, 0x83,
      0xc1, 0x60, 0x30, 0x18, 0xcc, 0xa1, 0xce, 0x88, 0x54, 0x94, 0x46, 0xe1, 0xb0, 0xd0, 0x4e, 0xb2, 0xf7, 0x04, 0x00};
  memset(st, 0, sizeof(*st));
  memcpy(st->cmd_depths, kDefaultCommandDepths, sizeof(kDefaultCommandDepths));
  memcpy(st->cmd_bits, kDefaultCommandBits, sizeof(kDefaultCommandBits));
  memcpy(st->cmd_code, kDefaultCommandCode, sizeof(kDefaultCommandCode));
  st->cmd_code_numbits = 448;
}

// ensure_initialized as far as this path needs it (encode.rs:657-707): the window bits become the open byte(s)
void Start(const EncoderParams& p, FragmentStream* fs) {
  if (fs->started) return;
  fs->started = true;
  const int lgwin = std::max(p.lgwin, 18);  // (quality 0 / 1, encode.rs:683-685)
  uint32_t bits = 0, n = 0;
  if (p.catable && p.bare_stream) {  // (no stream header, encode.rs:686-688)
  } else if (p.large_window) {
    bits = (uint32_t)(((lgwin & 0x3F) << 8) | 0x11);
    n = 14;
  } else if (lgwin == 16) {
    bits = 0;
    n = 1;
  } else if (lgwin == 17) {
    bits = 1;
    n = 7;
  } else if (lgwin > 17) {
    bits = (uint32_t)(((lgwin - 17) << 1) | 1);
    n = 4;
  } else {
    bits = (uint32_t)(((lgwin - 8) << 4) | 1);
    n = 7;
  }
  fs->last_bytes = (uint16_t)bits;
  fs->last_bytes_bits = (uint8_t)n;
  InitCommandPrefixCodes(&fs->state);
}

// HashTableSize / GetHashTable, encode.rs:1643-1700
uint32_t TableBits(int quality, size_t input_size) {
  const size_t max_table_size = quality == 0 ? ((size_t)1 << 15) : ((size_t)1 << 17);
  size_t htsize = 256;
  while (htsize < max_table_size && htsize < input_size) htsize <<= 1;
  if (quality == 0 && (htsize & 0xaaaaa) == 0) htsize <<= 1;
  uint32_t bits = 0;
  while (((size_t)1 << bits) < htsize) ++bits;
  return bits;
}

}  // namespace

bool IsFragmentStream(const EncoderParams& user_params) {
  EncoderParams p = user_params;
  FinalizeParams(&p);
  return (p.quality == 0 || p.quality == 1) && !p.catable;
}

namespace {

// The largest table_bits a fragment keeps in workgroup memory when it runs in a batch; 0 = never.  One setting per process, read
// once; by default, and at most, the largest the kernel takes (fragment_api.h).
uint32_t WorkgroupTableBits() {
  static const uint32_t v = [] {
    const char* s = getenv("BROTLI_MI355X_BATCH_LDS_BITS");
    if (!s) return (uint32_t)kFragmentWorkgroupTableBitsMax;
    return (uint32_t)std::min<unsigned long>(strtoul(s, nullptr, 10), kFragmentWorkgroupTableBitsMax);
  }();
  return v;
}

// One stream's share of a plan: `size` bytes of input behind what the stream has seen so far; `finish`: its last fragment carries
// is_last.  Whole bytes of output are appended to *out, the open byte stays in *fs.
struct FragmentWork {
  FragmentStream* fs;
  const uint8_t* input;
  size_t size;
  bool finish;
  std::vector<uint8_t>* out;
};

// A run of fragments of one stream inside a group, and the group: what goes to the device side by side.
struct FragmentRun {
  size_t work;      // index into the plan's work list
  size_t at, size;  // the input bytes [at, at + size) of that work
  bool last;        // the run ends the work's input (its last fragment carries is_last if the work finishes the stream)
  uint32_t first_job = 0, jobs = 0;
};
struct FragmentGroup {
  std::vector<FragmentRun> runs;
  size_t in_bytes = 0, slot_bytes = 0, table_words = 0, cmd_words = 0, lit_bytes = 0, jobs = 0;
};

size_t SlotBytes(size_t in_size) { return (2 * in_size + 520 + 63) & ~(size_t)63; }

// The fragments of every work of the list (cut at 1 << lgwin, as compress_stream_fast cuts one call's input; one block of the
// ring-buffer path is a single fragment), side by side on the device (fragment_api.h), whatever stream they belong to: streams are
// independent, and the fragments of one stream hang together through the bit position and (quality 0) the command code only.
// They go in groups of whole fragments: at most 4096 of them, about 256 MiB of input and 512 MiB of per-fragment scratch (hash
// table + command + literal buffers: about 1.1 MiB per fragment of >= 128 KiB) -- at least one fragment: device memory stays
// bounded however much one call hands over, slabs and grid dimensions stay bounded when the fragments are tiny.  A stream whose
// fragments do not fit one group goes on in the next.  Every fragment has scratch of its own size (no stride of the largest), and
// a fragment whose table is small enough for workgroup memory has no table slab at all.
void RunFragments(const EncoderParams& p, const std::vector<FragmentWork>& works) {
  const size_t block_size_limit = (size_t)1 << p.lgwin;
  static const size_t batch_target = getenv("BROTLI_MI355X_FRAGMENT_BATCH") ? (size_t)strtoull(getenv("BROTLI_MI355X_FRAGMENT_BATCH"), nullptr, 10) : ((size_t)256 << 20);
  static const bool selftest = getenv("BROTLI_MI355X_SELFTEST") != nullptr;
  static const bool test_again = getenv("BROTLI_MI355X_TEST_FRAGMENT_AGAIN") != nullptr;  // every fragment off phase 0 takes the one-by-one path
  static const size_t scratch_budget = getenv("BROTLI_MI355X_FRAGMENT_SCRATCH") ? (size_t)strtoull(getenv("BROTLI_MI355X_FRAGMENT_SCRATCH"), nullptr, 10) : ((size_t)512 << 20);
  const size_t group_bytes = std::max<size_t>(1, batch_target / block_size_limit) * block_size_limit;
  const bool q0 = p.quality == 0;
  // (a single stream keeps the kernel it always had: the workgroup table is for the small items of a batch)
  const uint32_t wg_bits = works.size() > 1 ? WorkgroupTableBits() : 0;
  auto table_words_of = [&](size_t block_size) {
    const uint32_t bits = TableBits(p.quality, block_size);
    return bits <= wg_bits ? (size_t)0 : (size_t)1 << bits;
  };
  auto cmd_words_of = [&](size_t block_size) { return q0 ? (size_t)0 : (std::min<size_t>(block_size, (size_t)1 << 17) + 16 + 3) & ~(size_t)3; };
  auto lit_bytes_of = [&](size_t block_size) { return q0 ? (size_t)0 : (std::min<size_t>(block_size, (size_t)1 << 17) + 64 + 15) & ~(size_t)15; };
  // ---- the plan: groups of runs
  std::vector<FragmentGroup> groups;
  for (size_t w = 0; w < works.size(); ++w) {
    const FragmentWork& work = works[w];
    size_t at = 0;
    for (;;) {
      const size_t block_size = std::min(block_size_limit, work.size - at);
      const bool ends = at + block_size == work.size;
      if (block_size == 0 && !(ends && work.finish)) break;
      const size_t scratch = 4 * table_words_of(block_size) + 4 * cmd_words_of(block_size) + lit_bytes_of(block_size);
      if (groups.empty() || groups.back().jobs == 4096 ||
          (groups.back().jobs != 0 && (groups.back().in_bytes + block_size > group_bytes ||
                                       4 * groups.back().table_words + 4 * groups.back().cmd_words + groups.back().lit_bytes + scratch > scratch_budget)))
        groups.emplace_back();
      FragmentGroup& g = groups.back();
      if (g.runs.empty() || g.runs.back().work != w) g.runs.push_back({w, at, 0, false, (uint32_t)g.jobs, 0});
      FragmentRun& run = g.runs.back();
      run.size += block_size;
      run.jobs++;
      run.last = ends;
      g.jobs++;
      g.in_bytes += block_size;
      g.slot_bytes += SlotBytes(block_size);
      g.table_words += table_words_of(block_size);
      g.cmd_words += cmd_words_of(block_size);
      g.lit_bytes += lit_bytes_of(block_size);
      at += block_size;
      if (ends) break;
    }
  }
  if (groups.empty()) return;
  // ---- device memory of the largest group, once
  FragmentGroup cap;
  size_t max_runs = 0;
  for (const FragmentGroup& g : groups) {
    cap.in_bytes = std::max(cap.in_bytes, g.in_bytes);
    cap.slot_bytes = std::max(cap.slot_bytes, g.slot_bytes);
    cap.table_words = std::max(cap.table_words, g.table_words);
    cap.cmd_words = std::max(cap.cmd_words, g.cmd_words);
    cap.lit_bytes = std::max(cap.lit_bytes, g.lit_bytes);
    cap.jobs = std::max(cap.jobs, g.jobs);
    max_runs = std::max(max_runs, g.runs.size());
  }
  const size_t max_jobs = cap.jobs;
  FragmentBuffers B;
  DevBlocks mem;
  uint8_t* const in = mem.zeroed<uint8_t>(cap.in_bytes + 64);
  // (behind the slots: the open bytes the runs come in with, 8 bytes each -- they are joined like any other piece)
  uint8_t* const slots = mem.uninit<uint8_t>(cap.slot_bytes + 8 * max_runs + 64);
  B.table = mem.uninit<uint32_t>(cap.table_words * 4 + 64);
  uint32_t* const commands = mem.uninit<uint32_t>(cap.cmd_words * 4 + 64);
  uint8_t* const literals = mem.uninit<uint8_t>(cap.lit_bytes + 64);
  B.commands = q0 ? nullptr : commands;
  B.literals = q0 ? nullptr : literals;
  // quality 0: [0, K) the distinct codes the runs come in with, [K + a] what fragment a of pass A leaves behind
  FragmentState* const sa = mem.uninit<FragmentState>((max_jobs + max_runs) * sizeof(FragmentState) + 64);
  FragmentState* const sb = mem.uninit<FragmentState>(max_jobs * sizeof(FragmentState) + 64);  // what fragment j leaves behind (pass B)
  FragmentJob* const jobs_dev = mem.uninit<FragmentJob>(max_jobs * sizeof(FragmentJob) + 64);
  uint32_t* const order_dev = mem.uninit<uint32_t>(max_jobs * sizeof(uint32_t) + 64);
  FragmentResult* const results_dev = mem.uninit<FragmentResult>(max_jobs * sizeof(FragmentResult) + 64);
  FragmentPiece* const pieces_dev = mem.uninit<FragmentPiece>((2 * max_jobs + max_runs) * sizeof(FragmentPiece) + 64);
  std::vector<FragmentJob> jobs, pass_a;
  std::vector<uint32_t> a_of_job, order;
  std::vector<FragmentState> incoming;
  std::vector<uint32_t> incoming_of_run;
  std::vector<FragmentResult> results;
  std::vector<FragmentPiece> pieces;
  std::vector<uint8_t> staged, heads, bytes;
  std::vector<uint64_t> run_base, run_end;
  // the fragments of `list` (uploaded to jobs_dev), class by class: the small ones on workgroup tables, the rest on their slabs
  auto launch = [&](int quality, const std::vector<FragmentJob>& list, const FragmentState* states_in, FragmentState* states_out) {
    const uint32_t n = (uint32_t)list.size();
    dev_h2d(jobs_dev, list.data(), (size_t)n * sizeof(FragmentJob));
    uint32_t classes[kFragmentWorkgroupTableBitsMax + 2] = {0};  // [0] device tables, [b] workgroup tables of b bits
    auto class_of = [&](const FragmentJob& job) { return job.table_bits <= wg_bits ? job.table_bits : 0u; };
    for (const FragmentJob& job : list) classes[class_of(job)]++;
    if (classes[0] == n) {
      frag_compress_jobs(quality, in, jobs_dev, nullptr, n, 0, B, states_in, states_out, results_dev, slots);
      return;
    }
    uint32_t first[kFragmentWorkgroupTableBitsMax + 2], fill[kFragmentWorkgroupTableBitsMax + 2];
    for (uint32_t c = 0, at = 0; c < kFragmentWorkgroupTableBitsMax + 2; at += classes[c], ++c) first[c] = fill[c] = at;
    order.resize(n);
    for (uint32_t j = 0; j < n; ++j) order[fill[class_of(list[j])]++] = j;
    dev_h2d(order_dev, order.data(), (size_t)n * sizeof(uint32_t));
    for (uint32_t c = 0; c < kFragmentWorkgroupTableBitsMax + 2; ++c)
      if (classes[c]) frag_compress_jobs(quality, in, jobs_dev, order_dev + first[c], classes[c], c, B, states_in, states_out, results_dev, slots);
  };
  for (const FragmentGroup& g : groups) {
    const uint32_t n = (uint32_t)g.jobs, n_runs = (uint32_t)g.runs.size();
    // ---- staging: one upload, every run at its own offset
    if (g.in_bytes) {
      if (n_runs == 1) {
        dev_h2d_bulk(in, works[g.runs[0].work].input + g.runs[0].at, g.in_bytes);
      } else {
        staged.resize(g.in_bytes);
        size_t at = 0;
        for (const FragmentRun& run : g.runs) {
          if (run.size) memcpy(staged.data() + at, works[run.work].input + run.at, run.size);
          at += run.size;
        }
        dev_h2d_bulk(in, staged.data(), g.in_bytes);
      }
    }
    // ---- the fragments of this group
    jobs.clear();
    pass_a.clear();
    a_of_job.assign(n, ~0u);
    incoming.clear();
    incoming_of_run.clear();
    size_t at = 0, slot_at = 0, table_at = 0, cmd_at = 0, lit_at = 0;
    for (const FragmentRun& run : g.runs) {
      const FragmentWork& work = works[run.work];
      if (q0) {
        if (incoming.empty() || memcmp(&incoming.back(), &work.fs->state, sizeof(FragmentState)) != 0) incoming.push_back(work.fs->state);
        incoming_of_run.push_back((uint32_t)incoming.size() - 1);
      }
      size_t left = run.size;
      for (uint32_t k = 0; k < run.jobs; ++k) {
        const size_t block_size = std::min(block_size_limit, left);
        FragmentJob job;
        job.in_offset = (uint32_t)at;
        job.in_size = (uint32_t)block_size;
        job.is_last = (run.last && work.finish && k + 1 == run.jobs) ? 1u : 0u;
        job.table_bits = TableBits(p.quality, block_size);
        job.out_offset = slot_at;
        job.start_bits = 0;
        job.state_in = q0 ? incoming_of_run.back() : 0;
        job.table_offset = table_at;
        job.cmd_offset = cmd_at;
        job.lit_offset = lit_at;
        // the command code a fragment leaves behind is built from the commands of its own last block, whatever code it came in
        // with (compress_fragment.rs:1033-1044): pass A runs every fragment that has a successor in its run with the run's
        // incoming code to learn what each leaves behind, pass B runs them all with the right incoming codes.  (A stream of a
        // single fragment needs no pass A.)
        if (q0 && k + 1 < run.jobs) {
          a_of_job[jobs.size()] = (uint32_t)pass_a.size();
          pass_a.push_back(job);
        }
        jobs.push_back(job);
        slot_at += SlotBytes(block_size);
        table_at += table_words_of(block_size);
        cmd_at += cmd_words_of(block_size);
        lit_at += lit_bytes_of(block_size);
        at += block_size;
        left -= block_size;
      }
    }
    if (jobs.size() != n || slot_at > cap.slot_bytes || table_at > cap.table_words || cmd_at > cap.cmd_words || lit_at > cap.lit_bytes || at > cap.in_bytes)
      throw std::runtime_error("brotli_mi355x: fragment plan ran over its bound");
    // ---- side by side, each into its own slot from bit 0 on
    const uint32_t K = (uint32_t)incoming.size();
    if (q0) {
      dev_h2d(sa, incoming.data(), (size_t)K * sizeof(FragmentState));
      if (!pass_a.empty()) launch(0, pass_a, sa, sa + K);
      for (uint32_t j = 0; j < n; ++j)
        if (j > 0 && a_of_job[j - 1] != ~0u) jobs[j].state_in = K + a_of_job[j - 1];
    }
    launch(p.quality, jobs, sa, q0 ? sb : nullptr);
    results.resize(n);
    dev_d2h(results.data(), results_dev, (size_t)n * sizeof(FragmentResult));
    if (q0 && selftest && !pass_a.empty()) {
      std::vector<FragmentState> a(pass_a.size()), b(n);
      dev_d2h(a.data(), sa + K, a.size() * sizeof(FragmentState));
      dev_d2h(b.data(), sb, (size_t)n * sizeof(FragmentState));
      for (uint32_t j = 0; j < n; ++j)
        if (a_of_job[j] != ~0u && memcmp(&a[a_of_job[j]], &b[j], sizeof(FragmentState)) != 0) throw std::runtime_error("brotli_mi355x selftest: the command code a quality 0 fragment leaves behind depends on the code it came in with");
    }
    // ---- where the slots go in the streams.  A fragment's bits move with the phase up to its first jump to a byte boundary; what
    // comes behind lands on whole bytes.  The padding of that jump is the one thing of a fragment that depends on the phase, and it
    // reaches one decision -- "larger than stored raw?", which counts output bits: where the true phase turns that decision around,
    // the fragment is compressed again by itself at its true phase.  Every run has its own stretch of the joined buffer, which
    // starts with the open byte its stream comes in with.
    pieces.clear();
    heads.assign((size_t)8 * n_runs, 0);
    run_base.assign(n_runs, 0);
    run_end.assign(n_runs, 0);
    const size_t heads_at = (cap.slot_bytes + 7) & ~(size_t)7;
    uint64_t joined_bytes = 0, longest = 0;
    for (uint32_t r = 0; r < n_runs; ++r) {
      const FragmentRun& run = g.runs[r];
      FragmentStream* const fs = works[run.work].fs;
      const uint64_t base = joined_bytes * 8;
      run_base[r] = base;
      heads[(size_t)8 * r] = (uint8_t)fs->last_bytes;
      heads[(size_t)8 * r + 1] = (uint8_t)(fs->last_bytes >> 8);
      if (fs->last_bytes_bits) pieces.push_back({(uint64_t)(heads_at + 8 * r) * 8, base, fs->last_bytes_bits});
      uint64_t cur = base + fs->last_bytes_bits;
      for (uint32_t j = run.first_job; j < run.first_job + run.jobs; ++j) {
        FragmentResult res = results[j];
        if (res.bad) throw std::runtime_error("brotli_mi355x: fragment compressor failed");
        const uint32_t phase = (uint32_t)(cur & 7u);
        const uint64_t slot_bit = jobs[j].out_offset * 8;
        bool again = false;
        if (phase != 0 && res.decision_align != ~0ull) {
          const uint64_t a = res.decision_align;
          const uint64_t pad0 = (8 - (a & 7)) & 7, padt = (8 - ((phase + a) & 7)) & 7;
          const uint64_t total = res.decision_bits - pad0 + padt;
          const bool fall_back = total > 31 + ((uint64_t)jobs[j].in_size << 3);
          again = fall_back != (res.fell_back != 0);
        }
        if (test_again && phase != 0) again = true;
        if (again) {
          if (getenv("BROTLI_MI355X_DEBUG")) fprintf(stderr, "fragment %u of %u: compressed again at phase %u (the raw fall-back hangs on the padding)\n", j, n, phase);
          // (by itself, where it sat: its slabs, its incoming code, its result slot)
          FragmentJob one = jobs[j];
          one.start_bits = phase;
          dev_h2d(jobs_dev + j, &one, sizeof(FragmentJob));
          frag_compress_jobs(p.quality, in, jobs_dev + j, nullptr, 1, one.table_bits <= wg_bits ? one.table_bits : 0, B, sa, q0 ? sb + j : nullptr,
                             results_dev + j, slots);
          dev_d2h(&res, results_dev + j, sizeof(FragmentResult));
          if (res.bad) throw std::runtime_error("brotli_mi355x: fragment compressor failed");
          pieces.push_back({slot_bit + phase, cur, res.end_bits - phase});
          cur += res.end_bits - phase;
          longest = std::max(longest, res.end_bits);
          continue;
        }
        longest = std::max(longest, res.end_bits);
        if (res.first_align == ~0ull) {
          pieces.push_back({slot_bit, cur, res.end_bits});
          cur += res.end_bits;
        } else {
          const uint64_t a = res.first_align, a8 = (a + 7) & ~(uint64_t)7;
          if (a) pieces.push_back({slot_bit, cur, a});
          const uint64_t aligned = (cur + a + 7) & ~(uint64_t)7;
          if (res.end_bits > a8) pieces.push_back({slot_bit + a8, aligned, res.end_bits - a8});
          cur = aligned + (res.end_bits - a8);
        }
      }
      run_end[r] = cur;
      joined_bytes = (((cur >> 3) + 2) + 7) & ~(uint64_t)7;
      // (the code the stream goes on with: only a stream that has not finished needs it)
      if (q0 && run.jobs != 0 && !(run.last && works[run.work].finish)) dev_d2h(&fs->state, sb + (run.first_job + run.jobs - 1), sizeof(FragmentState));
    }
    // ---- the join, and every stream of the group back in one download
    DevBlocks join_mem;
    uint8_t* const joined = join_mem.zeroed<uint8_t>((size_t)joined_bytes + 64);
    if (!pieces.empty()) {
      dev_h2d(slots + heads_at, heads.data(), heads.size());
      dev_h2d(pieces_dev, pieces.data(), pieces.size() * sizeof(FragmentPiece));
      frag_join_bounded(slots, pieces_dev, (uint32_t)pieces.size(), joined, longest);
    }
    bytes.resize((size_t)joined_bytes);
    dev_d2h_bulk(bytes.data(), joined, bytes.size());
    for (uint32_t r = 0; r < n_runs; ++r) {
      const FragmentWork& work = works[g.runs[r].work];
      FragmentStream* const fs = work.fs;
      const size_t from = (size_t)(run_base[r] >> 3), to = (size_t)(run_end[r] >> 3);
      work.out->insert(work.out->end(), bytes.begin() + (ptrdiff_t)from, bytes.begin() + (ptrdiff_t)to);
      fs->last_bytes = (uint16_t)(bytes[to] | (bytes[to + 1] << 8));
      fs->last_bytes_bits = (uint8_t)(run_end[r] & 7);
      if (fs->last_bytes_bits != 0) fs->last_bytes &= (uint16_t)((1u << fs->last_bytes_bits) - 1u); else fs->last_bytes = 0;
    }
  }
}

void RunFragments(const EncoderParams& p, FragmentStream* fs, const uint8_t* input, size_t size, bool finish, std::vector<uint8_t>* out) {
  RunFragments(p, std::vector<FragmentWork>{{fs, input, size, finish, out}});
}

// inject_byte_padding_block, encode.rs:1541-1566: an empty metadata block seals the open byte
void InjectPadding(FragmentStream* fs, std::vector<uint8_t>* out) {
  if (fs->last_bytes_bits == 0) return;
  uint32_t seal = fs->last_bytes;
  uint32_t seal_bits = fs->last_bytes_bits;
  seal |= 0x6u << seal_bits;
  seal_bits += 6;
  out->push_back((uint8_t)seal);
  if (seal_bits > 8) out->push_back((uint8_t)(seal >> 8));
  if (seal_bits > 16) out->push_back((uint8_t)(seal >> 16));
  fs->last_bytes = 0;
  fs->last_bytes_bits = 0;
}

// bits composed on the host behind the open byte; whole bytes go to *out, the rest becomes the open byte again
struct HostBits {
  FragmentStream* fs;
  std::vector<uint8_t>* out;
  uint64_t acc;
  uint32_t n;
  HostBits(FragmentStream* f, std::vector<uint8_t>* o) : fs(f), out(o), acc(f->last_bytes), n(f->last_bytes_bits) {
    while (n >= 8) {  // (the window bits of a large-window stream are 14)
      out->push_back((uint8_t)acc);
      acc >>= 8;
      n -= 8;
    }
  }
  void put(uint32_t nbits, uint64_t bits) {
    for (uint32_t b = 0; b < nbits; ++b) {
      acc |= ((bits >> b) & 1ull) << n;
      if (++n == 8) flush_byte();
    }
  }
  void flush_byte() {
    out->push_back((uint8_t)acc);
    acc = 0;
    n = 0;
  }
  void align() {
    if (n != 0) flush_byte();
  }
  void bytes(const uint8_t* p, size_t count) { out->insert(out->end(), p, p + count); }  // (byte aligned)
  ~HostBits() {
    fs->last_bytes = (uint16_t)acc;
    fs->last_bytes_bits = (uint8_t)n;
  }
};

}  // namespace

void FragmentStreamCompress(const EncoderParams& user_params, FragmentStream* fs, const uint8_t* input, size_t size, bool finish, bool flush,
                            std::vector<uint8_t>* out) {
  EncoderParams p = user_params;
  FinalizeParams(&p);
  Start(p, fs);
  if (size != 0 || finish) RunFragments(p, fs, input, size, finish, out);
  if (flush) InjectPadding(fs, out);
}

void FragmentBatchCompress(const EncoderParams& user_params, size_t count, const uint8_t* const* inputs, const size_t* sizes,
                           std::vector<std::vector<uint8_t>>* outs) {
  EncoderParams p = user_params;
  FinalizeParams(&p);
  std::vector<FragmentStream> streams(count);
  std::vector<FragmentWork> works(count);
  outs->assign(count, std::vector<uint8_t>());
  for (size_t i = 0; i < count; ++i) {
    Start(p, &streams[i]);
    works[i] = {&streams[i], inputs[i], sizes[i], true, &(*outs)[i]};
  }
  RunFragments(p, works);
}

bool IsFragmentRing(const EncoderParams& user_params) {
  EncoderParams p = user_params;
  FinalizeParams(&p);
  return (p.quality == 0 || p.quality == 1) && p.catable;
}

void FragmentRingCompress(const EncoderParams& user_params, FragmentStream* fs, const uint8_t* input, size_t size, bool finish, bool flush,
                          std::vector<uint8_t>* out) {
  EncoderParams p = user_params;
  FinalizeParams(&p);
  Start(p, fs);
  const size_t block = (size_t)1 << p.lgblock;  // (ComputeLgBlock: lgwin at these qualities)
  size_t avail = size;
  bool processing = true;
  while (processing) {
    // copy_input_to_ring_buffer: up to the end of the input block
    const size_t room = fs->pending.size() >= block ? 0 : block - fs->pending.size();
    if (room != 0 && avail != 0) {
      const size_t n = std::min(room, avail);
      fs->pending.insert(fs->pending.end(), input + (size - avail), input + (size - avail) + n);
      fs->saw_input = true;
      fs->input_seen += n;
      avail -= n;
      continue;
    }
    if (!(room == 0 || finish || flush)) break;  // PROCESS with a block that is not full yet
    const bool is_last = avail == 0 && finish;
    const bool force_flush = avail == 0 && flush;
    // ---- encode_data, encode.rs:2214-2389
    if (fs->size_hint == 0) {  // update_size_hint, encode.rs:1604-1620
      const uint64_t total = (uint64_t)fs->pending.size() + avail;
      fs->size_hint = p.size_hint != 0 ? p.size_hint : (size_t)std::min<uint64_t>(total, (uint64_t)1 << 30);
    }
    size_t bytes = fs->pending.size(), skip = 0;
    {
      HostBits hb(fs, out);
      if (fs->first_mb == 0 && p.magic_number) {
        // BrotliWriteMetadataMetaBlock, brotli_bit_stream.rs:2853-2896
        uint8_t b128[10];
        size_t count = 0;
        uint64_t value = fs->size_hint;
        for (size_t index = 0; index < 10; ++index) {
          b128[index] = (uint8_t)(value & 0x7f);
          value >>= 7;
          count = index + 1;
          if (value != 0) b128[index] |= 0x80; else break;
        }
        hb.put(1, 0);
        hb.put(2, 3);
        hb.put(1, 0);
        hb.put(2, 1);
        hb.put(8, 3 + count);
        hb.align();
        const uint8_t magic[4] = {0xe1, 0x97, (uint8_t)((p.catable && !p.use_dictionary) ? 0x81 : (p.appendable ? 0x82 : 0x80)), 1};
        hb.bytes(magic, 4);
        hb.bytes(b128, count);
        fs->first_mb = 1;
      }
      if (fs->first_mb != 3 && bytes != 0) {
        // the first two bytes of a catable stream go out raw, in a meta-block of their own (encode.rs:2283-2333)
        const uint32_t n = (uint32_t)std::min<size_t>(2, bytes);
        hb.put(1, 0);
        hb.put(2, 0);
        hb.put(16, n - 1);
        hb.put(1, 1);
        hb.align();
        hb.bytes(fs->pending.data(), n);
        skip = n;
        bytes -= n;
        fs->flushed_raw += n;
        fs->first_mb = n >= 2 ? 3 : (fs->first_mb == 2 ? 3 : 2);
      }
    }
    if (!(bytes == 0 && !is_last)) RunFragments(p, fs, fs->pending.data() + skip, bytes, is_last, out);
    fs->pending.clear();
    if (force_flush) {
      InjectPadding(fs, out);
      processing = false;
    }
    if (is_last) processing = false;
  }
}

bool FragmentRingMetadataReturns(const FragmentStream& fs) {
  const uint64_t will_go_raw = fs.first_mb != 3 ? std::min<uint64_t>(2, fs.pending.size()) : 0;
  return fs.input_seen == fs.flushed_raw + will_go_raw;
}

void FragmentStreamMetadataHeader(const EncoderParams& user_params, FragmentStream* fs, size_t size, std::vector<uint8_t>* out) {
  EncoderParams p = user_params;
  FinalizeParams(&p);
  Start(p, fs);
  uint8_t header[16];
  memset(header, 0, sizeof(header));
  size_t ix = fs->last_bytes_bits;
  header[0] = (uint8_t)fs->last_bytes;
  header[1] = (uint8_t)(fs->last_bytes >> 8);
  fs->last_bytes = 0;
  fs->last_bytes_bits = 0;
  auto put = [&](uint32_t n, uint64_t bits) {
    for (uint32_t b = 0; b < n; ++b, ++ix)
      if ((bits >> b) & 1) header[ix >> 3] |= (uint8_t)(1u << (ix & 7));
  };
  put(1, 0);
  put(2, 3);
  put(1, 0);
  if (size == 0) {
    put(2, 0);
  } else {
    uint32_t nbits = 0;
    if (size > 1) {
      uint32_t v = (uint32_t)size - 1;
      while (v) {
        nbits++;
        v >>= 1;
      }
    }
    const uint32_t nbytes = (nbits + 7) / 8;
    put(2, nbytes);
    put(8 * nbytes, (uint64_t)size - 1);
  }
  out->insert(out->end(), header, header + ((ix + 7) >> 3));
}

}  // namespace brotli_mi355x
