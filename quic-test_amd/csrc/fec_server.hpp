// fec_server.hpp — the protocol of the resident legacy encoder's ring (fec_coalesce.cpp "resident
// server" on the host, fec_server.hip legacy_server on the device): the slot, control and
// coordination layouts, their constants and the arithmetic rules both sides and the CPU model
// (tests/csrc/ring_protocol_test.cpp) share.  Plain C++: no HIP include, so the model compiles
// with any host compiler; in a HIP compile the rules are __host__ __device__.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define QFEC_SERVER_HD __host__ __device__
#else
#define QFEC_SERVER_HD
#endif

namespace qfec {

// ---- resident legacy encoder (fec_coalesce.cpp "resident server") ----
// A ring of submission slots (page-locked coherent host memory, or VRAM written through the BAR).
// The host fills slot seq % kServerSlots with a legacy call's groups: every 8-B word of a slot
// carries the slot's tag, server_tag(seq), in its top 16 bits, so the device recognises a
// complete slot by the tags alone, whatever order its reads of the host's stores land in.  An
// aligned 8-B store is the unit the host's stores are assumed to arrive in (x86 quadword
// atomicity); nothing larger is assumed to arrive in one piece, so every 8-B word is
// self-validating.  Resident workgroups serve the slots in seq order (one per serving class,
// below) and store done[seq % kServerSlots] = seq + 1.  Calls are served without a kernel launch
// each.
//
// Tags and the epoch.  A slot's tag is (lap & (epoch - 1)) + 1 with lap = seq / kServerSlots and
// epoch a power of two (no division on the server's critical path), so the tags of one slot
// repeat every `epoch` laps (32768; shorter in the test library, fec_knobs.hpp kResidentEpoch).  A word left from the previous epoch could carry the current tag (a word written
// exactly `epoch` laps ago and not since, e.g. a later group's address word under inline-only
// calls), so the slot is scrubbed at every epoch boundary: the server zeroes the slot's words
// and its inline data area after serving the last lap of an epoch, before that slot's done word
// (its next occupant writes only after it has seen the done word, so the zeroes are in place
// first), and the host zeroes the slot's inline output staging before publishing the first lap
// of an epoch.  Within an epoch every tag of a slot is used once, so no stale word matches;
// tag 0 (the zeroed state) never matches.
constexpr uint32_t kServerSlots = 1024;
constexpr uint32_t kServerMaxGroups = 8;  // groups per slot (legacy calls of 1..8 groups)
constexpr uint32_t kServerPackets = 10;   // the legacy call's packets per group
constexpr uint64_t kServerTagShift = 48;  // addresses below 2^48 (x86-64 user virtual addresses)
constexpr uint64_t kServerAddrMask = (1ull << kServerTagShift) - 1;
constexpr uint32_t kServerEpoch = 32768;  // laps per tag epoch, a power of two (tags 1 .. epoch fit 16 bits)
QFEC_SERVER_HD inline uint32_t server_tag(uint64_t seq, uint32_t epoch) {
  return (static_cast<uint32_t>(seq / kServerSlots) & (epoch - 1u)) + 1u;
}
// Whether the server scrubs the slot of seq after serving it (the last lap of an epoch).
QFEC_SERVER_HD inline bool server_scrub_after(uint64_t seq, uint32_t epoch) {
  return (static_cast<uint32_t>(seq / kServerSlots) & (epoch - 1u)) == epoch - 1u;
}
struct alignas(64) ServerSlot {
  uint64_t out;             // tag | device address of the repair rows, row g at out + g * P
  uint64_t shape;           // tag | P (bits 0..15) | groups (bits 16..23; 0 = nothing to do) | kServerInline
  uint64_t addr[kServerMaxGroups * kServerPackets];  // tag | device address of packet (g, j) at [g * 10 + j]
};
// VRAM ring (large-BAR devices, fec_coalesce.cpp Resident): the slots and the packets of small
// calls live in uncached device memory that the host writes through the BAR, so the server's
// poll and packet loads stay on the device.  An inline slot (shape bit kServerInline) carries
// no addresses: its packets are copied by the host into the slot's data area, packet (g, j) as
// 16-B chunks at chunk (g * 10 + j) * nch + c, nch = ceil(P / 12).  A chunk is two 8-B halves,
// each 6 payload bytes and the slot's 16-bit tag in its top two bytes:
//   bytes 0..5 = payload [12c, 12c + 6), bytes 6..7 = tag, bytes 8..13 = payload [12c + 6,
//   12c + 12), bytes 14..15 = tag (payload zero past P),
// so each half validates itself (a 16-B write-combined store may reach the device as two 8-B
// pieces) and no ordering of the host's stores through the BAR is assumed.  The rows come back
// the same way: an inline slot's `out` is its output staging in page-locked host memory, repair
// chunk (g, c) in the same two-half form at out + (g * nch + c) * 16, and the host takes the rows
// once both halves of every chunk carry the tag (the done word then only says "consumed").
constexpr uint64_t kServerInline = 1ull << 24;
constexpr uint32_t kInlineMaxGroups = 4;
constexpr uint32_t kInlineMaxP = 1536;
constexpr uint32_t kInlinePayload = 12;  // payload bytes of a 16-B chunk (6 per 8-B half)
constexpr uint32_t kInlineSlotBytes = kInlineMaxGroups * kServerPackets * (kInlineMaxP / kInlinePayload) * 16;
// Serving classes.  An instance is `classes` workgroups (a power of two, 1 .. kServerMaxClasses,
// so it divides kServerSlots): workgroup c serves the seqs with seq % classes == c, in order, so
// concurrent callers are served by independent poll -> serve -> done cycles.
constexpr uint32_t kServerMaxClasses = 8;
constexpr uint32_t kServerPoll = 16;  // slots of its class a workgroup reads per poll (the longest run it serves)
struct alignas(64) ServerControl {
  uint64_t stop;            // host -> device: leave at the next poll
  uint64_t pad0[7];
  uint64_t exited;          // device -> host: generation of the last instance that left (its last workgroup)
  uint64_t pad1[7];
  uint64_t progress[kServerMaxClasses];   // device -> host: every seq of class c below progress[c] was served
  uint64_t bad_slots[kServerMaxClasses];  // device -> host: polls that found a slot with a word not yet landed (diagnostic)
  uint64_t scrubs[kServerMaxClasses];     // device -> host: slots scrubbed at an epoch boundary (diagnostic)
};
// Device memory the workgroups of one instance share (uncached: they run on different XCDs, each
// with its own L2).  Words are tagged with the instance's generation, so nothing is reset
// between instances.
struct alignas(64) ServerCoord {
  uint64_t leave;                      // gen: every workgroup of instance gen leaves at its next poll
  uint64_t exits;                      // (gen << 8) | workgroups of instance gen that have left
  uint64_t pad[6];
  uint64_t idle[kServerMaxClasses];    // gen while class c's workgroup has been idle for idle_ticks, else 0
};
// The coordination rules, shared by legacy_server and the CPU model (tests/csrc/ring_protocol_test.cpp).
// Whether every class of instance gen is idle: this one (idle, now) and the others by the flags
// it last read (idle_seen[c] == gen; a flag of an earlier instance never counts).
QFEC_SERVER_HD inline bool server_all_idle(bool idle, const uint64_t* idle_seen, uint32_t classes, uint32_t cls,
                                           uint64_t gen) {
  bool all = idle;
  for (uint32_t c = 0; c < classes; ++c) all = all && (c == cls || idle_seen[c] == gen);
  return all;
}
// The exit count: a workgroup leaving instance gen turns the word v into this (the word still
// holds the previous instance's count until the first of this one's); the workgroup whose new
// word counts all `classes` is the last out and stores ctl->exited = gen.
QFEC_SERVER_HD inline uint64_t server_exits_next(uint64_t v, uint64_t gen) {
  return (v >> 8) == gen ? v + 1 : (gen << 8) | 1u;
}
QFEC_SERVER_HD inline bool server_exits_last(uint64_t nv, uint32_t classes) { return (nv & 0xFFu) == classes; }

}  // namespace qfec

#undef QFEC_SERVER_HD
