// pcb_model — cgck_pcb_build and cgck_pcb_lookup on the CPU, one entry and one
// frame at a time, through the probe text the kernels compile
// (con-gen_amd/csrc/cgck_pcb_probe.h) over an accessor of plain arrays.  Built with
// -fsanitize=address,undefined (tools/Makefile), so every index the probe text
// hands to an accessor is checked against the arrays' real bounds; the arrays are
// heap blocks of exactly their size.  tests/test_pcb_cpu.py runs it over the corpus
// of tests/pcbbatches.py and compares with tests/pcbref.py.
//
//	pcb_model IN OUT MODE      MODE: cgck_test_pcb_mode's bits
//
// IN: nine u32 (magic, nconn, nflow, n, bound present, cls present, buffer bytes, 0,
// 0), then conn, flow, bound, desc, seg, cls, buf.  OUT: stat u32[4], idx u32[n],
// fidx u32[n], kind u8[n], count u32[6].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../con-gen_amd/csrc/cgck_pcb_probe.h"
#include "cgck.h"

using namespace cgck;

// The accessor: heap arrays of exactly the size the file gives.
struct Host {
	uint32_t nconn, nflow;
	const uint8_t *conn_, *flow_;
	uint64_t *t64;
	uint32_t *t32;

	void conn(uint32_t j, uint32_t &flow, uint32_t &ports, uint32_t &w2) const
	{
		uint32_t w[3];
		memcpy(w, conn_ + 12 * (size_t)j, 12);
		flow = w[0], ports = w[1], w2 = w[2];
	}
	void flow_key(uint32_t f, uint32_t &flags, uint32_t (&a)[8]) const
	{
		flags = flow_[48 * (size_t)f + 14];
		memcpy(a, flow_ + 48 * (size_t)f + 16, 32);
	}
	uint64_t slot64(uint32_t s) const { return t64[s]; }
	uint32_t slot32(uint32_t s) const { return t32[s]; }
	uint64_t cas64(uint32_t s, uint64_t v)
	{
		const uint64_t seen = t64[s];
		if (seen == kPcbEmpty64)
			t64[s] = v;
		return seen;
	}
	uint32_t cas32(uint32_t s, uint32_t v)
	{
		const uint32_t seen = t32[s];
		if (seen == kPcbNone)
			t32[s] = v;
		return seen;
	}
	void min64(uint32_t s, uint64_t v) { t64[s] = v < t64[s] ? v : t64[s]; }
	void min32(uint32_t s, uint32_t v) { t32[s] = v < t32[s] ? v : t32[s]; }
};

static uint8_t *slurp(FILE *f, size_t bytes)
{
	uint8_t *p = (uint8_t *)malloc(bytes ? bytes : 1);
	if (!p || fread(p, 1, bytes, f) != bytes) {
		fprintf(stderr, "pcb_model: short input\n");
		exit(2);
	}
	return p;
}

template <bool TAG>
static void run(Host &a, uint32_t mask, bool chain, uint32_t n, const uint8_t *desc, const uint8_t *seg, const uint8_t *cls,
		const uint8_t *bound, const uint8_t *buf, size_t buf_bytes, uint32_t *stat, uint32_t *idx, uint32_t *fidx,
		uint8_t *kind, uint32_t *count)
{
	// the build: the entries in index order (any order gives the same table contents per key)
	for (uint32_t i = 0; i < a.nconn; ++i) {
		PcbKey key;
		uint32_t flow;
		const int st = pcb_conn_key(a, i, key, flow);
		if (st != kPcbValid) {
			stat[st == kPcbUnused ? 2 : 3] += 1;
			continue;
		}
		const uint32_t h = pcb_hash(key);
		uint32_t s = pcb_home(h, mask, chain);
		for (uint32_t it = 0; it <= mask; ++it) {
			const int r = pcb_insert_step<TAG>(a, i, key, h, s);
			if (r != kPcbGo) {
				stat[r == kPcbPlaced ? 0 : 1] += 1;
				break;
			}
			s = (s + 1) & mask;
		}
	}
	// the lookup
	for (uint32_t k = 0; k < n; ++k) {
		uint64_t off;
		uint16_t l3, len, sport, dport;
		memcpy(&off, desc + 12 * (size_t)k, 8);
		memcpy(&l3, desc + 12 * (size_t)k + 8, 2);
		memcpy(&len, desc + 12 * (size_t)k + 10, 2);
		memcpy(&sport, seg + 32 * (size_t)k + 16, 2);
		memcpy(&dport, seg + 32 * (size_t)k + 18, 2);
		if (off + l3 + len > buf_bytes) {
			fprintf(stderr, "pcb_model: frame %u lies past the buffer\n", k);
			exit(2);
		}
		const uint8_t *b = buf + off + l3;
		const uint32_t c = cls ? cls[k] & 15u : (uint32_t)CGCK_SEG_TCP;
		idx[k] = fidx[k] = kPcbNone;
		const uint32_t v = len ? b[0] >> 4 : 0u;
		if (c != CGCK_SEG_TCP && c != CGCK_SEG_UDP) {
			kind[k] = CGCK_PCB_SKIP;
		} else if (len == 0 || !((v == 4 && len >= 20) || (v == 6 && len >= 40))) {
			kind[k] = CGCK_PCB_NONE;
		} else {
			PcbKey key = {};
			memcpy(key.a, b + (v == 6 ? 24 : 16), v == 6 ? 16 : 4);
			memcpy(key.a + 4, b + (v == 6 ? 8 : 12), v == 6 ? 16 : 4);
			key.ports = dport | (uint32_t)sport << 16;
			key.fp = (v == 6 ? 1u : 0u) | (c == CGCK_SEG_UDP ? 17u : 6u) << 8;
			const uint32_t h = pcb_hash(key);
			uint32_t s = pcb_home(h, mask, chain);
			kind[k] = CGCK_PCB_MISS;
			for (uint32_t it = 0; a.nconn != 0 && it <= mask; ++it) {
				const int r = pcb_probe_step<TAG>(a, key, h, s, idx[k], fidx[k]);
				if (r == kPcbHit)
					kind[k] = CGCK_PCB_HIT;
				if (r != kPcbGo)
					break;
				s = (s + 1) & mask;
			}
			if (kind[k] != CGCK_PCB_HIT)
				fidx[k] = kPcbNone;
			const uint32_t port = (dport & 255u) << 8 | dport >> 8;
			if (kind[k] == CGCK_PCB_MISS && bound && port < CGCK_PCB_NBOUND) {
				uint32_t w;
				memcpy(&w, bound + 4 * (size_t)port, 4);
				if (w != kPcbNone) {
					kind[k] = CGCK_PCB_BOUND;
					idx[k] = w;
				}
			}
			if (kind[k] == CGCK_PCB_HIT && v == 6)
				count[5] += 1;
		}
		count[kind[k]] += 1;
	}
}

int main(int argc, char **argv)
{
	if (argc != 4) {
		fprintf(stderr, "usage: pcb_model IN OUT MODE\n");
		return 2;
	}
	const int mode = atoi(argv[3]);
	FILE *f = fopen(argv[1], "rb");
	uint32_t hd[9];
	if (mode < 0 || mode > 3 || !f || fread(hd, 4, 9, f) != 9 || hd[0] != 0x42435043u || hd[1] > (1u << 24)) {
		fprintf(stderr, "pcb_model: bad arguments or header\n");
		return 2;
	}
	const uint32_t nconn = hd[1], nflow = hd[2], n = hd[3];
	uint8_t *conn = slurp(f, 12 * (size_t)nconn), *flow = slurp(f, 48 * (size_t)nflow);
	uint8_t *bound = hd[4] ? slurp(f, 4 * (size_t)CGCK_PCB_NBOUND) : nullptr;
	uint8_t *desc = slurp(f, 12 * (size_t)n), *seg = slurp(f, 32 * (size_t)n);
	uint8_t *cls = hd[5] ? slurp(f, n) : nullptr;
	uint8_t *buf = slurp(f, hd[6]);
	fclose(f);

	const bool tagged = !(mode & 2);
	const uint32_t slots = pcb_slots(nconn);
	if (cgck_pcb_table_bytes(nconn) != (size_t)slots * 8)
		return 3;
	// the table is exactly the bytes the shape uses, filled as the launcher fills it
	const size_t tbytes = (size_t)slots * (tagged ? 8 : 4);
	void *table = malloc(tbytes);
	memset(table, 0xFF, tbytes);
	Host a = {nconn, nflow, conn, flow, (uint64_t *)table, (uint32_t *)table};
	std::vector<uint32_t> idx(n), fidx(n);
	std::vector<uint8_t> kind(n);
	uint32_t stat[4] = {}, count[CGCK_PCB_NCOUNT] = {};
	if (tagged)
		run<true>(a, slots - 1, mode & 1, n, desc, seg, cls, bound, buf, hd[6], stat, idx.data(), fidx.data(), kind.data(), count);
	else
		run<false>(a, slots - 1, mode & 1, n, desc, seg, cls, bound, buf, hd[6], stat, idx.data(), fidx.data(), kind.data(), count);

	FILE *o = fopen(argv[2], "wb");
	if (!o)
		return 2;
	fwrite(stat, 4, 4, o);
	fwrite(idx.data(), 4, n, o);
	fwrite(fidx.data(), 4, n, o);
	fwrite(kind.data(), 1, n, o);
	fwrite(count, 4, CGCK_PCB_NCOUNT, o);
	fclose(o);
	for (void *p : {(void *)conn, (void *)flow, (void *)bound, (void *)desc, (void *)seg, (void *)cls, (void *)buf, table})
		free(p);
	return 0;
}
