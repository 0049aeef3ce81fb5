// cgck_pcb_probe.h — the probe text of cgck_pcb_build / cgck_pcb_lookup
// (include/cgck.h, section 3): the private hash, the slot arithmetic, the key
// compare, the insert step and the probe step, as inline functions over a small
// accessor.  The kernels (cgck_pcb.hip) compile it for the device with an
// accessor of global loads and atomics; tools/pcb_model.cpp compiles the same text
// for the CPU with an accessor over plain arrays, under the sanitizers.  Plain
// C++: no HIP header is needed to read it.
//
// Table.  Open addressing, linear probing, `mask + 1` slots, a power of two of at
// least 2 nconn (pcb_slots), so an empty slot always exists.  A slot holds a
// connection's index, never its key: keys are read from conn[] and flow[], which
// nobody writes, so no reader ever waits for a writer and a reported match is a
// match of the arrays.  Two shapes share this text:
//   TAG   8-byte slots, tag << 32 | idx, tag the key's whole 32-bit hash; a probe
//         fetches conn[] and flow[] only behind an equal tag;
//   !TAG  4-byte slots, the index alone: half the table, a key fetch per occupied
//         slot probed.
// An empty slot is all ones in both (idx < 2^30 keeps an occupied one apart).
//
// An accessor A has
//	uint32_t nconn, nflow;
//	void conn(uint32_t j, uint32_t &flow, uint32_t &ports, uint32_t &w2) const;   // conn[j]'s three dwords
//	void flow_key(uint32_t f, uint32_t &flags, uint32_t (&a)[8]) const;           // flow[f].flags, laddr, faddr
//	uint64_t slot64(uint32_t s) const;  uint32_t slot32(uint32_t s) const;
//	uint64_t cas64(uint32_t s, uint64_t v);  uint32_t cas32(uint32_t s, uint32_t v);   // empty -> v; the value found
//	void min64(uint32_t s, uint64_t v);  void min32(uint32_t s, uint32_t v);
// and checks nothing: every index is compared with nconn or nflow here before the
// accessor sees it.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define CGCK_PCB_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define CGCK_PCB_HD inline
#endif

namespace cgck {

constexpr uint32_t kPcbMaxConn = 1u << 30;
constexpr uint32_t kPcbNone = 0xFFFFFFFFu;
constexpr uint64_t kPcbEmpty64 = ~(uint64_t)0;
constexpr uint32_t kPcbFlowBits = 3; // CGCK_FLOW_IP6 | CGCK_FLOW_VLAN
constexpr uint32_t kPcbFlowIp6 = 1;

// Slots of the table for nconn <= kPcbMaxConn entries: the power of two at or
// above 2 nconn, at least 2.  Both shapes use this count; cgck_pcb_table_bytes is
// 8 bytes a slot, what the tagged shape needs.
constexpr uint32_t pcb_slots(uint32_t nconn)
{
	uint32_t s = 2;
	while (s < 2 * nconn)
		s *= 2;
	return s;
}

// (family, proto, laddr, faddr, lport, fport).  An IPv4 key has a[1..3] and
// a[5..7] zero, so equal IPv4 tuples are equal keys whatever bytes 4..15 of the
// flow record hold.
struct PcbKey {
	uint32_t a[8];  // laddr, faddr as the wire bytes read little-endian
	uint32_t ports; // lport | fport << 16, as stored
	uint32_t fp;    // family (1: IPv6) | proto << 8
};

CGCK_PCB_HD uint32_t pcb_rotl(uint32_t x, int r)
{
	return x << r | x >> (32 - r);
}

// The private hash: every field of the key goes in (MurmurHash3's 32-bit rounds
// and finalizer), laddr and proto included, which SO_HASH leaves out.
CGCK_PCB_HD uint32_t pcb_hash(const PcbKey &k)
{
	uint32_t h = 0x9747b28cu;
	const uint32_t w[10] = {k.fp, k.ports, k.a[0], k.a[1], k.a[2], k.a[3], k.a[4], k.a[5], k.a[6], k.a[7]};
	for (int i = 0; i < 10; ++i) {
		uint32_t x = w[i] * 0xcc9e2d51u;
		x = pcb_rotl(x, 15) * 0x1b873593u;
		h = pcb_rotl(h ^ x, 13) * 5u + 0xe6546b64u;
	}
	h ^= 40u;
	h = (h ^ h >> 16) * 0x85ebca6bu;
	h = (h ^ h >> 13) * 0xc2b2ae35u;
	return h ^ h >> 16;
}

// The slot a key's probe starts at.  chain (cgck_test_pcb_mode bit 0): the
// table's last slot for every key, the longest chain and the wrap-around.
CGCK_PCB_HD uint32_t pcb_home(uint32_t h, uint32_t mask, bool chain)
{
	return chain ? mask : h & mask;
}

enum { kPcbValid = 0, kPcbUnused = 1, kPcbBadFlow = 2 };

// The key of connection j < nconn and its flow index; kPcbUnused (proto 0) and
// kPcbBadFlow (flow >= nflow, or a flag bit outside IP6 | VLAN) have no key.
template <class A>
CGCK_PCB_HD int pcb_conn_key(const A &a, uint32_t j, PcbKey &k, uint32_t &flow)
{
	uint32_t ports, w2;
	a.conn(j, flow, ports, w2);
	const uint32_t proto = w2 & 255u;
	if (proto == 0)
		return kPcbUnused;
	if (flow >= a.nflow)
		return kPcbBadFlow;
	uint32_t flags;
	a.flow_key(flow, flags, k.a);
	if (flags & ~kPcbFlowBits)
		return kPcbBadFlow;
	if (!(flags & kPcbFlowIp6))
		k.a[1] = k.a[2] = k.a[3] = k.a[5] = k.a[6] = k.a[7] = 0;
	k.ports = ports;
	k.fp = (flags & kPcbFlowIp6) | proto << 8;
	return kPcbValid;
}

// Connection j < nconn is valid and its key is `want` (want.fp's proto is never
// 0).  The ports and the protocol are judged before flow[] is read.
template <class A>
CGCK_PCB_HD bool pcb_conn_matches(const A &a, uint32_t j, const PcbKey &want, uint32_t &flow)
{
	uint32_t f, ports, w2;
	a.conn(j, f, ports, w2);
	if (ports != want.ports || (w2 & 255u) != want.fp >> 8 || f >= a.nflow)
		return false;
	uint32_t flags, b[8];
	a.flow_key(f, flags, b);
	if ((flags & ~kPcbFlowBits) != 0 || (flags & kPcbFlowIp6) != (want.fp & 1u))
		return false;
	bool eq = b[0] == want.a[0] && b[4] == want.a[4];
	if (flags & kPcbFlowIp6)
		eq = eq && b[1] == want.a[1] && b[2] == want.a[2] && b[3] == want.a[3] && b[5] == want.a[5] &&
		     b[6] == want.a[6] && b[7] == want.a[7];
	flow = f;
	return eq;
}

enum { kPcbGo = 0, kPcbHit = 1, kPcbEnd = 2 };

// One step of a lookup at slot s: kPcbHit with idx and flow set, kPcbEnd at an
// empty slot, kPcbGo to move on to (s + 1) & mask.  The caller counts the steps
// and stops after mask + 1.  An index the table holds is used only when it is
// below nconn, and a hit is a compare of conn[] and flow[]: a table of any bytes
// costs hits, never a fault or a false hit.
template <bool TAG, class A>
CGCK_PCB_HD int pcb_probe_step(const A &a, const PcbKey &want, uint32_t h, uint32_t s, uint32_t &idx, uint32_t &flow)
{
	uint32_t j;
	if (TAG) {
		const uint64_t v = a.slot64(s);
		if (v == kPcbEmpty64)
			return kPcbEnd;
		if ((uint32_t)(v >> 32) != h)
			return kPcbGo;
		j = (uint32_t)v;
	} else {
		j = a.slot32(s);
		if (j == kPcbNone)
			return kPcbEnd;
	}
	if (j >= a.nconn || !pcb_conn_matches(a, j, want, flow))
		return kPcbGo;
	idx = j;
	return kPcbHit;
}

enum { kPcbPlaced = 1, kPcbDup = 2 };

// One step of the insert of valid connection i (key, h = pcb_hash(key)) at slot
// s: kPcbPlaced when i took the empty slot, kPcbDup when the slot's occupant has
// i's key (the lower index stays: an atomic min), kPcbGo to move on.
//
// Why this needs no waiting.  A slot goes from empty to occupied once and never
// back, and what replaces an occupant has the occupant's key (the min below), so
// "occupied by another key" is final the moment it is seen.  The slot is read
// first and the compare-and-swap is tried only on a slot seen empty: a stale
// "empty" merely fails the swap, which returns the occupant.  All entries of one
// key walk the same slots from the same home and pass the same occupants, so they
// meet in the first slot one of them takes; the lowest index survives there
// whatever the order.
template <bool TAG, class A>
CGCK_PCB_HD int pcb_insert_step(A &a, uint32_t i, const PcbKey &key, uint32_t h, uint32_t s)
{
	uint32_t j, flow;
	if (TAG) {
		const uint64_t mine = (uint64_t)h << 32 | i;
		uint64_t v = a.slot64(s);
		if (v == kPcbEmpty64) {
			v = a.cas64(s, mine);
			if (v == kPcbEmpty64)
				return kPcbPlaced;
		}
		if ((uint32_t)(v >> 32) != h)
			return kPcbGo;
		j = (uint32_t)v;
		if (j >= a.nconn || !pcb_conn_matches(a, j, key, flow))
			return kPcbGo;
		a.min64(s, mine);
	} else {
		j = a.slot32(s);
		if (j == kPcbNone) {
			j = a.cas32(s, i);
			if (j == kPcbNone)
				return kPcbPlaced;
		}
		if (j >= a.nconn || !pcb_conn_matches(a, j, key, flow))
			return kPcbGo;
		a.min32(s, i);
	}
	return kPcbDup;
}

} // namespace cgck
