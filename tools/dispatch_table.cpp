// dispatch_table — checks choose() (con-gen_amd/csrc/cgck_choose.cpp) against a
// recorded decision table (tests/golden/dispatch.txt; dispatch_lab.txt for the
// build with -DCGCK_LAB=1).  Host arithmetic only: it links neither libcgck nor
// HIP and never opens a GPU.
//
//   dispatch_table FIXTURE
//
// The fixture: `#` comment lines, one `columns` line naming the (pin, bits)
// columns as PIN:BITS (decimal; bits = kPacked | kExplicit | kNT | kContig |
// kStrOld), then rows
//
//   FLAGS LENS SHAPES OUTPUTS TOKENS
//
// each standing for every batch of the cross product of its first four fields
// (batches with the same recorded answers share a row).  FLAGS: hex flag sets
// (public and internal bits), comma-separated; LENS: packet lengths (also the
// length hint), comma-separated; SHAPES, comma-separated: s0..s3 strided with
// stride = len rounded up to 16 / len + 2 / 2048 / 0 with l3_off 14, d-
// descriptors 16-byte aligned, u- descriptors at +4; OUTPUTS, one letter each:
// a `out` aligned, u `out` at +4, v aligned with verdicts, b aligned with bad
// counters.  TOKENS holds one character per column: kAlphabet[kernel * 4 + nt +
// 2 * contig], kernel in the order of kKernelNames; nt reads 0 for a kernel
// whose launcher takes no nt argument.
//
// Prints one line per mismatch (inputs -> got / expected), then the number of
// cases and mismatches and, per kernel of this build, the cases the fixture
// expects on it.  Exit status 1 when anything mismatches, 2 on a bad fixture.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../con-gen_amd/csrc/cgck_choose.h"

using namespace cgck;

static const char kAlphabet[] = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz+-*/=?@%";
// Every Kernel value of this build, in the order the tokens count them.
static const struct {
	Kernel kernel;
	const char *name;
	bool takes_nt;
} kKernelNames[] = {
	{Kernel::kGroup, "group", true}, {Kernel::kLpp, "lpp", true},   {Kernel::kSlot2, "slot2", true},
	{Kernel::kLpa, "lpa", true},     {Kernel::kLpd, "lpd", false},  {Kernel::kLpw, "lpw", false},
	{Kernel::kLpw6, "lpw6", false},  {Kernel::kLpf, "lpf", false},  {Kernel::kDstr, "dstr", false},
#if CGCK_LAB
	{Kernel::kSlot, "slot", true},   {Kernel::kLppp, "lppp", true}, {Kernel::kLpp0, "lpp0", true},
	{Kernel::kLpp1, "lpp1", true},   {Kernel::kLpp3, "lpp3", true}, {Kernel::kSpan, "span", true},
	{Kernel::kSlotd, "slotd", false}, {Kernel::kStream, "stream", false},
#endif
};
constexpr int kKernels = sizeof(kKernelNames) / sizeof(kKernelNames[0]);
static_assert(sizeof(kAlphabet) - 1 >= 4u * kKernels, "a character per (kernel, nt, contig)");

// The token of a choice; -1 for a kernel this build does not know.
static int token_of(const Choice &c)
{
	for (int k = 0; k < kKernels; ++k)
		if (kKernelNames[k].kernel == c.kernel)
			return 4 * k + (c.nt && kKernelNames[k].takes_nt) + 2 * c.contig;
	return -1;
}

// The batch a row stands for.  Addresses are never dereferenced.
static bool batch_of(unsigned flags, unsigned len, char kind, char layout, char outs, KParams *p)
{
	*p = KParams{};
	p->base = reinterpret_cast<const uint8_t *>(0x10000000);
	p->n = 4096;
	p->flags = flags;
	if (kind == 's') {
		p->ip_len = len;
		switch (layout) {
		case '0': p->stride = (len + 15) & ~15u; break;
		case '1': p->stride = len + 2; break;
		case '2': p->stride = 2048; break;
		case '3': p->stride = 0, p->l3_off = 14; break;
		default: return false;
		}
	} else if ((kind == 'd' || kind == 'u') && layout == '-') {
		p->desc = reinterpret_cast<const cgck_desc_t *>(kind == 'd' ? 0x20000000 : 0x20000004);
	} else {
		return false;
	}
	p->out = reinterpret_cast<uint32_t *>(outs == 'u' ? 0x30000004 : 0x30000000);
	if (outs == 'v')
		p->verdict = reinterpret_cast<uint8_t *>(0x40000000);
	if (outs == 'b')
		p->bad = reinterpret_cast<uint32_t *>(0x50000000);
	return outs == 'a' || outs == 'u' || outs == 'v' || outs == 'b';
}

static std::string describe(int token)
{
	if (token < 0 || token >= 4 * kKernels)
		return "(no kernel of this build)";
	return std::string(kKernelNames[token / 4].name) + (token & 1 ? " nt" : "") + (token & 2 ? " contig" : "");
}

static std::vector<std::string> split(const char *list)
{
	std::vector<std::string> out(1);
	for (; *list; ++list)
		if (*list == ',')
			out.emplace_back();
		else
			out.back() += *list;
	return out;
}

int main(int argc, char **argv)
{
	FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
	if (!f) {
		fprintf(stderr, "usage: dispatch_table FIXTURE\n");
		return 2;
	}
	std::vector<std::pair<int, int>> cols; // pin, bits
	long cases = 0, mismatches = 0, reached[kKernels] = {};
	char line[4096];
	for (int lineno = 1; fgets(line, sizeof(line), f); ++lineno) {
		if (line[0] == '#' || line[0] == '\n')
			continue;
		if (!strncmp(line, "columns", 7)) {
			int pin, bits, used;
			for (const char *s = line + 7; sscanf(s, " %d:%d%n", &pin, &bits, &used) == 2; s += used)
				cols.emplace_back(pin, bits);
			continue;
		}
		char flagsets[256], lens[256], shapes[64], outputs[16], tokens[256];
		bool ok = sscanf(line, "%255s %255s %63s %15s %255s", flagsets, lens, shapes, outputs, tokens) == 5 &&
			  strlen(tokens) == cols.size();
		for (const std::string &fs : split(flagsets))
			for (const std::string &ls : split(lens))
				for (const std::string &shape : split(shapes))
					for (const char *o = outputs; ok && *o; ++o) {
						const unsigned flags = (unsigned)strtoul(fs.c_str(), nullptr, 16);
						const unsigned len = (unsigned)strtoul(ls.c_str(), nullptr, 10);
						KParams p;
						if (!(ok = shape.size() == 2 && batch_of(flags, len, shape[0], shape[1], *o, &p)))
							break;
						for (size_t i = 0; i < cols.size(); ++i, ++cases) {
							const char *at = strchr(kAlphabet, tokens[i]);
							const int want = at ? (int)(at - kAlphabet) : -1;
							const int got = token_of(choose(p, len, cols[i].first | cols[i].second));
							if (want >= 0 && want < 4 * kKernels)
								++reached[want / 4];
							if (got == want)
								continue;
							++mismatches;
							printf("flags 0x%x len %u shape %s outputs %c pin %d bits %d -> got %s / expected %s\n",
							       flags, len, shape.c_str(), *o, cols[i].first, cols[i].second,
							       describe(got).c_str(), describe(want).c_str());
						}
					}
		if (!ok) {
			fprintf(stderr, "%s:%d: malformed row\n", argv[1], lineno);
			return 2;
		}
	}
	fclose(f);
	printf("cases %ld mismatches %ld\n", cases, mismatches);
	for (int k = 0; k < kKernels; ++k)
		printf("reached %s %ld\n", kKernelNames[k].name, reached[k]);
	return mismatches ? 1 : 0;
}
