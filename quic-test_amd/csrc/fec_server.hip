// fec_server.hip — gfx950 (MI355X, CDNA4) kernel of libfec_hip: legacy_server, the resident
// encoder that serves legacy calls from a ring of submission slots without a kernel launch each
// (fec_coalesce.cpp "resident server").  The ring's protocol -- the slot, control and coordination
// words, the tags and their epoch, the serving classes -- is fec_server.hpp's, shared with the
// host side and the CPU model (tests/csrc/ring_protocol_test.cpp); this file holds the kernel,
// its system-scope loads and stores and its launcher.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fec_device.hpp"  // u32x4, u32x4u
#include "fec_kernels.hpp"
#include "fec_knobs.hpp"
#include "fec_launch.hpp"  // launch_record

namespace qfec {
namespace {

// Resident legacy encoder (fec_server.hpp ServerSlot): workgroups of 16 waves, one per serving
// class (below).  One poll
// is one round trip over PCIe: 128 lanes read the first two 64-B lines of each of the next 16
// slots (the header words and the first group's 10 packet addresses, 16 B a lane: 32 line reads
// in all -- reading every word of 64 slots separately took 5 us a poll, 2x a round trip); a
// slot is complete when every one of those words carries its lap tag, and the run of complete
// slots from the next expected seq is served (slots in order).  Then every thread takes work
// items (one 16-B column of one group: its 10 packets loaded, XORed -- the reference's row 0,
// fec_xor_simd.cpp:411-427 -- and stored to the repair row), the workgroup fences its stores
// at system scope and the slots' done words are stored (release).  Every wave leaves together:
// at the host's stop flag, after idle_ticks without work, after life_ticks, and in any case
// after kServerMaxPolls polls.
constexpr uint32_t kServerThreads = 1024;
constexpr uint32_t kServerMaxPolls = 1u << 22;
constexpr uint32_t kServerHeadWords = 16;  // words of a slot read by the poll: out, shape, addr[0..13]

__device__ __forceinline__ void sys_store_release(uint64_t* p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// System-coherent (uncached) access for the words the host polls: program order with the
// system-coherent stores before them, and vmcnt(0) in between, is the ordering.
__device__ __forceinline__ void sys_store_relaxed(uint64_t* p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// 16 bytes to host memory at any address, written system-coherent (sc0 sc1: write-through, no
// cache keeps a copy), so legacy_server's vmcnt(0) after its repair-row stores means the rows
// are in host memory before it stores the done words (no release fence;
// profiles/r03_resident_store_ab.txt).  That is the gfx94x / gfx95x ISA's meaning of sc0 sc1,
// not the HIP memory model's guarantee: a build for another target stops here.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__)
#error "legacy_server assumes gfx94x/gfx95x sc0 sc1 stores are write-through (sys_store_16b)"
#endif
// Written as the instruction itself: a volatile store compiles to the same instruction but is
// followed by s_waitcnt vmcnt(0), one PCIe acknowledgement per store before the thread goes on
// (the VRAM ring's stamps: 1.7 us a batch spent there).  The server's own vmcnt(0) before its
// done words is the one wait the rows need; the "memory" clobber keeps the compiler's memory
// operations on their side of it, and an extra outstanding store only makes the compiler's own
// vmcnt waits (in-order completion on gfx9) stricter.
__device__ __forceinline__ void sys_store_16b(uint8_t* p, u32x4 v) {
  __asm__ volatile("global_store_dwordx4 %0, %1, off sc0 sc1" : : "v"(p), "v"(v) : "memory");
}

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

// The server's workgroup barrier: every value it publishes between its waves is in LDS, so the
// fences are LDS-only (s_waitcnt lgkmcnt(0) + s_barrier).  __syncthreads' workgroup fence also
// waits vmcnt(0) -- the PCIe acknowledgement of every repair-row store, which an inline batch
// does not need (its rows carry lap words) and an addressed batch waits for explicitly.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// 16 bytes of host memory as they are now (system-coherent load, no cache).
__device__ __forceinline__ u64x2 sys_load_16(const uint64_t* p) {
  return *reinterpret_cast<const volatile __attribute__((address_space(1))) u64x2*>(reinterpret_cast<uintptr_t>(p));
}

// The VRAM ring (inl != nullptr, fec_server.hpp kServerInline): the poll reads the slots from
// device memory -- local, not a PCIe round trip -- and an inline slot's work item is one 16-B
// chunk column (g, c): its 10 chunks loaded from the slot's data area (or, at the head of the
// run, from the poll's prefetch), the tags of both 8-B halves of each checked, the 12 payload
// bytes XORed and stored with the tag in both halves as chunk (g, c) of the slot's output
// staging.  A half whose tag is not yet this slot's (the host's stores through the BAR landed
// in another order, or a 16-B store arrived as two pieces) marks the slot bad: the run is served
// up to the first bad slot and the poll comes back for the rest.  The host takes an inline
// slot's rows by their tags, so its done word needs no acknowledgement of the row stores: a
// batch of inline slots only waits for them when it also holds an addressed slot (or scrubs a
// slot at an epoch boundary, fec_server.hpp server_tag).
//
// Serving classes (fec_server.hpp kServerMaxClasses): workgroup c of `classes` serves the seqs
// of class c (seq % classes == c) and steps through them `classes` apart; its poll, run, done
// words and progress mark are its class's alone.  The workgroups share only the ServerCoord
// words (uncached device memory, read with the poll): an idle flag each, and the leave word any
// of them sets when it leaves on its own (the stop word, the life bound, its poll bound) or finds
// every class idle -- so an instance leaves as a whole, and the last workgroup out stores the
// exited word the host relaunches on.
__global__ __launch_bounds__(kServerThreads) void legacy_server(ServerSlot* __restrict__ ring,
                                                                uint8_t* __restrict__ inl,
                                                                uint64_t* __restrict__ done,
                                                                ServerControl* __restrict__ ctl,
                                                                ServerCoord* __restrict__ coord, uint32_t classes,
                                                                uint64_t gen, uint64_t idle_ticks, uint64_t slow_ticks,
                                                                uint64_t life_ticks, uint64_t* __restrict__ stamps,
                                                                uint32_t epoch) {
  __shared__ uint64_t s_next;
  __shared__ uint32_t s_n, s_exit, s_stop, s_ack, s_told, s_slow;
  __shared__ uint64_t s_idle[kServerMaxClasses];
  __shared__ uint32_t s_first[kServerPoll + 1];  // work items before slot i of the run
  __shared__ uint32_t s_P[kServerPoll], s_cpp[kServerPoll], s_inl[kServerPoll], s_bad[kServerPoll];
  __shared__ uint64_t s_head[kServerPoll][kServerHeadWords];  // out, shape, addr[0..13] (tagged)
  const uint32_t K = classes, cls = blockIdx.x;
  // the shared words are read by every 8th poll (an instance leaves within 8 polls of the word)
  constexpr uint32_t kCoordEvery = 7u;
  if (cls != 0) stamps = nullptr;  // class 0's stamps only
  // VRAM ring: every poll also reads the first 16 KB of the next slot's inline data area, one
  // 16-B chunk a thread, in flight with the header loads -- an inline slot found complete at
  // the head of the run then takes its chunks from here instead of a second dependent round
  // trip to memory (1 group of P <= 1224: 10 * ceil(P / 12) chunks <= 1024).  Read before the
  // slot is known complete: the chunks' lap words decide, as for any chunk.
  __shared__ u32x4 s_pre[kServerThreads];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  uint64_t t0 = 0, t_last = 0;  // thread 0 only
  uint64_t n_bad = 0, n_scrub = 0;  // thread 0 only: the diagnostic counters, continued from the last instance's
  bool was_idle = false;            // thread 0 only: this class's idle flag as last published
  if (tid == 0) {
    // the class's first unserved seq: its progress mark (the first instance's marks are 0, so
    // rounded up into the class)
    const uint64_t p = *reinterpret_cast<const volatile uint64_t*>(&ctl->progress[cls]);
    s_next = p + (cls + K - static_cast<uint32_t>(p % K)) % K;
    t0 = t_last = static_cast<uint64_t>(wall_clock64());
    s_told = 0;
    for (uint32_t c = 0; c < kServerMaxClasses; ++c) s_idle[c] = 0;
    n_bad = *reinterpret_cast<const volatile uint64_t*>(&ctl->bad_slots[cls]);
    n_scrub = *reinterpret_cast<const volatile uint64_t*>(&ctl->scrubs[cls]);
  }
  lds_barrier();
  // Diagnostic stamps (stamps != nullptr; the test library's TestKnob::kResidentStamps): thread 0's wall clock at the
  // phases of each served batch, into a ring of 256 records of 8 words in host memory that no
  // other code reads; never part of a result.
  uint64_t st_batches = 0, st_polls = 0, st_t[7] = {};
  for (uint32_t it = 0; it < kServerMaxPolls; ++it) {
    const uint64_t next = s_next;
    if (stamps != nullptr && tid == 0) st_t[0] = static_cast<uint64_t>(wall_clock64());
    // the poll: the first two lines of each of the next kServerPoll slots, 16 B a lane, and the
    // host's stop word, all in one round trip
    u32x4 pre = {0u, 0u, 0u, 0u};
    if (inl != nullptr)
      pre = __builtin_nontemporal_load(reinterpret_cast<const __attribute__((address_space(1))) u32x4*>(
          reinterpret_cast<uintptr_t>(inl + static_cast<uint64_t>(next % kServerSlots) * kInlineSlotBytes) + tid * 16u));
    constexpr uint32_t kPollLanes = kServerPoll * kServerHeadWords / 2;
    if (tid < kPollLanes) {
      const uint32_t i = tid / (kServerHeadWords / 2), piece = tid % (kServerHeadWords / 2);
      const u64x2 v = sys_load_16(reinterpret_cast<const uint64_t*>(ring + (next + uint64_t(i) * K) % kServerSlots) + 2 * piece);
      s_head[i][2 * piece] = v.x;
      s_head[i][2 * piece + 1] = v.y;
    } else if (tid == kPollLanes) {
      // with the ring in VRAM the stop word (host memory) would make every poll a PCIe round
      // trip again: every 16th poll reads it (the idle and life bounds hold regardless)
      s_stop = (inl == nullptr || (it & 15u) == 0) ? (*reinterpret_cast<const volatile uint64_t*>(&ctl->stop) != 0 ? 1u : 0u)
                                                   : 0u;
    } else if (coord != nullptr && (it & kCoordEvery) == 0 && tid == kPollLanes + 1) {
      s_told = sys_load_16(&coord->leave).x == gen ? 1u : 0u;
    } else if (coord != nullptr && (it & kCoordEvery) == 0 && tid >= kPollLanes + 2 &&
               tid < kPollLanes + 2 + kServerMaxClasses / 2) {
      const uint32_t q = tid - (kPollLanes + 2);
      const u64x2 v = sys_load_16(&coord->idle[2 * q]);
      s_idle[2 * q] = v.x;
      s_idle[2 * q + 1] = v.y;
    }
    s_pre[tid] = pre;
    lds_barrier();
    if (tid < 64) {
      const uint64_t seq = next + uint64_t(lane) * K;
      const uint64_t tag = server_tag(seq, epoch);
      bool ok = lane < kServerPoll;
      bool inline_slot = false;
      if (ok) {
        // out, shape and (unless the packets are inline) the first group's 10 addresses (words 0 .. 11)
        inline_slot = inl != nullptr && (s_head[lane][1] & kServerInline) != 0;
        const uint32_t nw = inline_slot ? 2u : 2u + kServerPackets;
#pragma unroll
        for (uint32_t w = 0; w < 2 + kServerPackets; ++w) ok = ok && (w >= nw || (s_head[lane][w] >> kServerTagShift) == tag);
        s_bad[lane] = 0;
      }
      const uint64_t bal = __ballot(ok);
      const uint32_t n = ~bal == 0 ? 64u : static_cast<uint32_t>(__builtin_ctzll(~bal));
      const uint64_t addressed = __ballot(lane < n && !inline_slot);  // rows straight to the caller
      uint32_t work = 0;
      if (lane < n) {
        const uint64_t sh = s_head[lane][1];
        const uint32_t P = static_cast<uint32_t>(sh & 0xFFFFu), G = static_cast<uint32_t>((sh >> 16) & 0xFFu);
        const uint32_t cpp = inline_slot ? (P + kInlinePayload - 1u) / kInlinePayload : (P + 15u) / 16u;
        s_P[lane] = P;
        s_cpp[lane] = cpp;
        s_inl[lane] = inline_slot ? 1u : 0u;
        // (an inline shape past the data area is never written by the host: nothing is read for it)
        work = inline_slot && (G > kInlineMaxGroups || P > kInlineMaxP) ? 0u : G * cpp;
      }
      uint32_t incl = work;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(incl, d, 64);
        if (lane >= static_cast<uint32_t>(d)) incl += y;
      }
      if (lane < kServerPoll) s_first[lane + 1] = incl;
      if (lane == 0) {
        s_first[0] = 0;
        const uint64_t now = static_cast<uint64_t>(wall_clock64());
        if (n > 0) t_last = now;
        const bool stop = s_stop != 0;
        s_n = n;
        s_ack = addressed != 0 ? 1u : 0u;
        const bool idle = n == 0 && now - t_last > idle_ticks;
        // (class 0, where the host puts a lone caller's calls, never polls slowly)
        s_slow = cls != 0 && n == 0 && now - t_last > slow_ticks ? 1u : 0u;
        bool leave = stop || now - t0 > life_ticks || it + 1 == kServerMaxPolls;
        if (coord == nullptr) {
          leave = leave || idle;
        } else {
          // every class idle (this one now, the others by their published flags), or told to leave
          const bool all_idle = server_all_idle(idle, s_idle, K, cls, gen);
          if (idle != was_idle) {
            sys_store_relaxed(&coord->idle[cls], idle ? gen : 0);
            was_idle = idle;
          }
          if ((leave || all_idle) && s_told == 0) sys_store_relaxed(&coord->leave, gen);
          leave = leave || all_idle || s_told != 0;
        }
        s_exit = leave ? 1u : 0u;
      }
    }
    lds_barrier();
    const uint32_t n = s_n;
    const bool leave = s_exit != 0;
    if (stamps != nullptr && tid == 0) {
      st_t[1] = static_cast<uint64_t>(wall_clock64());
      ++st_polls;
    }
    if (n > 0) {
      // the packets (and any later groups' addresses) as the host wrote them before the words above
      // The caller's packets as the host wrote them before its slot (the L2 may hold an older
      // copy of the same lines from an earlier call).  Cached loads after this acquire: reading
      // the packets system-coherent instead (sc0 sc1, no fence) made every 16-B load its own
      // PCIe read and the work step 2.8x slower (12.6 vs 4.5 us a batch).
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
      if (stamps != nullptr && tid == 0) st_t[2] = st_t[6] = static_cast<uint64_t>(wall_clock64());  // (a bad slot: no item)
      const uint32_t total = s_first[n];
      for (uint32_t w = tid; w < total; w += kServerThreads) {
        uint32_t i = 0;
        while (s_first[i + 1] <= w) ++i;
        const uint32_t local = w - s_first[i];
        const uint32_t cpp = s_cpp[i], P = s_P[i];
        const uint32_t g = local / cpp, col = local - g * cpp;
        const uint64_t seq = next + uint64_t(i) * K;
        if (s_inl[i] != 0) {
          const uint32_t c0 = g * kServerPackets * cpp + col;  // chunk (g, 0, col)
          u32x4 v[kServerPackets];
          if (i == 0 && (g + 1) * kServerPackets * cpp <= kServerThreads) {
            // the head of the run: the poll brought its chunks
#pragma unroll
            for (uint32_t j = 0; j < kServerPackets; ++j) v[j] = s_pre[c0 + j * cpp];
          } else {
            const uint8_t* src = inl + static_cast<uint64_t>(seq % kServerSlots) * kInlineSlotBytes + c0 * 16u;
#pragma unroll
            for (uint32_t j = 0; j < kServerPackets; ++j)
              v[j] = *reinterpret_cast<const __attribute__((address_space(1))) u32x4*>(
                  reinterpret_cast<uintptr_t>(src + static_cast<uint64_t>(j) * cpp * 16u));
#pragma unroll
            for (uint32_t j = 0; j < kServerPackets; ++j) __asm__ volatile("" : "+v"(v[j]));
          }
          // both 8-B halves of every chunk carry this lap's tag in their top two bytes
          const uint32_t tag = server_tag(seq, epoch);
          bool fresh = true;
          u32x4 acc = v[0];
#pragma unroll
          for (uint32_t j = 0; j < kServerPackets; ++j) fresh = fresh && (v[j].y >> 16) == tag && (v[j].w >> 16) == tag;
#pragma unroll
          for (uint32_t j = 1; j < kServerPackets; ++j) acc ^= v[j];
          if (!fresh) {
            s_bad[i] = 1u;
            continue;
          }
          if (stamps != nullptr && tid == 0 && w == 0) st_t[6] = static_cast<uint64_t>(wall_clock64());
          // tagged rows, whole 16-B pieces side by side: a wave's stores cover whole lines (three
          // 32-bit stores per 12 bytes, each writing every third word of a line, took 31 us a
          // call instead of 6.9: every batch was found only by the poll that also read the stop
          // word from host memory -- the partial-line writes and the done word behind them left
          // the device only when a read to the host pushed them; profiles/r04_vram_store_forms.txt)
          sys_store_16b(reinterpret_cast<uint8_t*>(s_head[i][0] & kServerAddrMask) + (static_cast<uint64_t>(g) * cpp + col) * 16u,
                        u32x4{acc.x, (acc.y & 0xFFFFu) | (tag << 16), acc.z, (acc.w & 0xFFFFu) | (tag << 16)});
          continue;
        }
        const uint32_t coff = col * 16u + 16u <= P ? col * 16u : P - 16u;
        uint64_t ad[kServerPackets];
        if (g == 0) {
#pragma unroll
          for (uint32_t j = 0; j < kServerPackets; ++j) ad[j] = s_head[i][2 + j];
        } else {
          // written by the host before the slot's first group and header, seen complete above;
          // relaxed system-scope loads (uncached, all ten in flight: volatile loads were each
          // followed by a full wait, one PCIe round trip apiece)
          const uint64_t* src = ring[seq % kServerSlots].addr + g * kServerPackets;
#pragma unroll
          for (uint32_t j = 0; j < kServerPackets; ++j)
            ad[j] = __hip_atomic_load(reinterpret_cast<const __attribute__((address_space(1))) uint64_t*>(
                                          reinterpret_cast<uintptr_t>(src + j)),
                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          // tagged like the header: in a VRAM ring the host's stores through the BAR carry no
          // order, and a word of the previous lap marks the slot bad (served by a later poll)
          const uint64_t tag = server_tag(seq, epoch);
          bool fresh = true;
#pragma unroll
          for (uint32_t j = 0; j < kServerPackets; ++j) fresh = fresh && (ad[j] >> kServerTagShift) == tag;
          if (!fresh) {
            s_bad[i] = 1u;
            continue;
          }
        }
        // All ten packet loads in flight at once, as global (address space 1) loads: the addresses
        // come from integers, so plain pointers compile to flat loads, which count on lgkmcnt too
        // and were issued two at a time with a full wait between pairs -- five dependent PCIe
        // round trips, ~8 us of a ~12-us call (the server's stamps, DESIGN_HISTORY.md §8c round 4).
        u32x4 v[kServerPackets];
#pragma unroll
        for (uint32_t j = 0; j < kServerPackets; ++j)
          v[j] = *reinterpret_cast<const __attribute__((address_space(1))) u32x4u*>((ad[j] & kServerAddrMask) + coff);
#pragma unroll
        for (uint32_t j = 0; j < kServerPackets; ++j) __asm__ volatile("" : "+v"(v[j]));  // no load sunk into the XOR
        u32x4 acc = v[0];
#pragma unroll
        for (uint32_t j = 1; j < kServerPackets; ++j) acc ^= v[j];
        if (stamps != nullptr && tid == 0 && w == 0) {  // thread 0's packet loads have returned
          __asm__ volatile("" : "+v"(acc));
          st_t[6] = static_cast<uint64_t>(wall_clock64());
        }
        uint8_t* dst = reinterpret_cast<uint8_t*>(s_head[i][0] & kServerAddrMask) + static_cast<uint64_t>(g) * P + coff;
        sys_store_16b(dst, acc);
      }
      if (stamps != nullptr && tid == 0) st_t[3] = static_cast<uint64_t>(wall_clock64());
      // The repair rows were stored system-coherent (no cache to write back): wait until every
      // one of this thread's stores is acknowledged, then the workgroup's barrier, then the done
      // words -- no release fence.  Same box, alternating (profiles/r03_resident_store_ab.txt):
      // one caller 8.0 vs 10.9 us a call, 16 callers 550k vs 330k calls/s against plain stores
      // and a system release fence (its L2 write-back 1.7-2.9 us a batch).  Not for a batch of
      // inline slots only: their rows carry lap words, and their done words only say the slot
      // was consumed (its loads have returned).
      if (s_ack != 0) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
      if (stamps != nullptr && tid == 0) st_t[4] = static_cast<uint64_t>(wall_clock64());
      lds_barrier();
      // the run up to its first slot with a word not yet landed (n when every word had)
      uint32_t n_ok = n;
      bool scrub = false;
      for (uint32_t k = 0; k < n; ++k) {
        if (s_bad[k] != 0) {
          n_ok = k;
          break;
        }
        scrub = scrub || server_scrub_after(next + uint64_t(k) * K, epoch);
      }
      if (tid == 0 && n_ok < n) sys_store_relaxed(&ctl->bad_slots[cls], ++n_bad);
      if (scrub) {
        // The last lap of an epoch (fec_server.hpp server_tag): zero the served slot's words and
        // inline data area before its done word, so no word of this epoch can match a tag of the
        // next.  Its next occupant writes only after it has seen the done word.
        constexpr uint32_t kSlotPieces = sizeof(ServerSlot) / 16u;
        const uint32_t pieces = kSlotPieces + (inl != nullptr ? kInlineSlotBytes / 16u : 0u);
        for (uint32_t k = 0; k < n_ok; ++k) {
          const uint64_t seq = next + uint64_t(k) * K;
          if (!server_scrub_after(seq, epoch)) continue;
          uint8_t* slot = reinterpret_cast<uint8_t*>(ring + seq % kServerSlots);
          uint8_t* area = inl != nullptr ? inl + (seq % kServerSlots) * kInlineSlotBytes : nullptr;
          for (uint32_t c = tid; c < pieces; c += kServerThreads)
            sys_store_16b(c < kSlotPieces ? slot + c * 16u : area + (c - kSlotPieces) * 16u, u32x4{0u, 0u, 0u, 0u});
          if (tid == 0) ++n_scrub;
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): every zero in place before the done words
        lds_barrier();
        if (tid == 0) sys_store_relaxed(&ctl->scrubs[cls], n_scrub);
      }
      if (tid < n_ok) {
        const uint64_t seq = next + uint64_t(tid) * K;
        sys_store_relaxed(&done[seq % kServerSlots], seq + 1);
      }
      if (tid == 0) {
        s_next = next + uint64_t(n_ok) * K;
        sys_store_relaxed(&ctl->progress[cls], next + uint64_t(n_ok) * K);
      }
      if (stamps != nullptr && tid == 0) {
        st_t[5] = static_cast<uint64_t>(wall_clock64());
        uint64_t* rec = stamps + (st_batches % 256) * 8;
        rec[0] = st_t[1] - st_t[0];  // the poll that found the run
        rec[1] = st_t[2] - st_t[1];  // decision + acquire fence
        rec[2] = st_t[6] - st_t[2];  // thread 0's first work item: its 10 packet loads
        rec[3] = st_t[3] - st_t[6];  // its store (and any further items)
        rec[4] = st_t[5] - st_t[3];  // stores acknowledged + barrier + done stores
        rec[5] = n;
        rec[6] = st_polls;           // polls since the previous batch, this one included
        __threadfence_system();
        sys_store_release(&rec[7], ++st_batches);
        st_polls = 0;
      }
    } else if (!leave) {
      // a class other than 0 without work for slow_ticks polls every ~5 us instead of every ~1.5
      // (the host gives a lone caller's calls to class 0, whose polls other classes' polls slow down)
      if (s_slow != 0)
        __builtin_amdgcn_s_sleep(127);
      else
        __builtin_amdgcn_s_sleep(8);
    }
    lds_barrier();
    if (leave) break;
  }
  if (tid == 0) {
    sys_store_release(&ctl->progress[cls], s_next);
    bool last = true;
    if (coord != nullptr) {
      // count this workgroup out of instance gen (the word still holds the previous instance's
      // count until the first of this one's); at most `classes` contenders, so the loop ends
      uint64_t v = __hip_atomic_load(&coord->exits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM), nv = 0;
      do {
        nv = server_exits_next(v, gen);
      } while (!__hip_atomic_compare_exchange_strong(&coord->exits, &v, nv, __ATOMIC_ACQ_REL, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_SYSTEM));
      last = server_exits_last(nv, K);
    }
    if (last) sys_store_release(&ctl->exited, gen);
  }
}

}  // namespace

// The launcher: checks the instance's arguments, then one launch of `classes` workgroups.
hipError_t launch_legacy_server(ServerSlot* ring, uint8_t* inl, uint64_t* done, ServerControl* ctl,
                                ServerCoord* coord, uint32_t classes, uint64_t gen, uint64_t idle_ticks,
                                uint64_t slow_ticks, uint64_t life_ticks, uint64_t* stamps, uint32_t epoch,
                                hipStream_t s) {
  if (epoch < 1u || epoch > kServerEpoch || (epoch & (epoch - 1u)) != 0) return hipErrorInvalidValue;
  // classes: a power of two (it divides kServerSlots), with the shared words when more than one;
  // gen fits the exit count's 56 bits
  if (classes < 1u || classes > kServerMaxClasses || (classes & (classes - 1u)) != 0 || (classes > 1u && !coord) ||
      gen == 0 || gen >= (1ull << 56))
    return hipErrorInvalidValue;
  trace_launch(launch_record(LaunchForm::kLegacyServer, classes, kServerThreads, 0, 0));
  hipLaunchKernelGGL(legacy_server, dim3(classes), dim3(kServerThreads), 0, s, ring, inl, done, ctl,
                     classes > 1u ? coord : nullptr, classes, gen, idle_ticks, slow_ticks, life_ticks, stamps, epoch);
  return hipGetLastError();
}

hipError_t load_server_unit() {
  hipFuncAttributes at;
  return hipFuncGetAttributes(&at, reinterpret_cast<const void*>(legacy_server));
}

}  // namespace qfec
