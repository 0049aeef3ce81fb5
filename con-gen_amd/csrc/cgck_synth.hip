// cgck_synth.hip — device-side synthetic batches and the
// streaming-read diagnostics probes.
#include "cgck_device.h"

namespace cgck {

// --------------------------------------------------------------------------
// Synthetic input: byte j of the stream = byte j&7 of
// splitmix64(seed, j>>3); then per-packet header stamps.
// --------------------------------------------------------------------------

__device__ __forceinline__ uint64_t splitmix64(uint64_t seed, uint64_t j)
{
	uint64_t z = seed + (j + 1) * 0x9e3779b97f4a7c15ull;
	z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
	z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
	return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void synth_fill_kernel(uint8_t *base, uint64_t nbytes, uint64_t seed)
{
	const uint64_t nw = nbytes >> 3;
	uint64_t *w = reinterpret_cast<uint64_t *>(base);
	for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; 2 * i < nw;
	     i += (uint64_t)gridDim.x * 256) {
		uint64_t j = 2 * i;
		if (j + 1 < nw) {
			ulonglong2 x = make_ulonglong2(splitmix64(seed, j), splitmix64(seed, j + 1));
			*reinterpret_cast<ulonglong2 *>(w + j) = x;
		} else {
			w[j] = splitmix64(seed, j);
		}
	}
	if (blockIdx.x == 0 && threadIdx.x < (nbytes & 7)) {
		uint64_t b = (nw << 3) + threadIdx.x;
		base[b] = (uint8_t)(splitmix64(seed, b >> 3) >> (8 * (b & 7)));
	}
}

__device__ __forceinline__ void stamp(uint8_t *ip, uint32_t len)
{
	ip[0] = 0x45;
	ip[1] = 0;
	ip[2] = (uint8_t)(len >> 8);
	ip[3] = (uint8_t)len;
	ip[9] = 6;
	ip[10] = 0;
	ip[11] = 0;
	if (len >= 38) {
		ip[36] = 0;
		ip[37] = 0;
	}
}

__global__ __launch_bounds__(256) void synth_stamp_strided_kernel(uint8_t *base, uint64_t n,
								  uint64_t stride, uint32_t len)
{
	for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n;
	     k += (uint64_t)gridDim.x * 256)
		stamp(base + k * stride, len);
}

// IPv6 stamp (cgck_synth_strided_ip6): version word, payload length, next
// header, and the checksum field of nh zeroed when the packet holds it.
__global__ __launch_bounds__(256) void synth_stamp6_strided_kernel(uint8_t *base, uint64_t n, uint64_t stride,
								   uint32_t len, uint32_t nh)
{
	const int fo = v6_field(nh);
	for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (uint64_t)gridDim.x * 256) {
		uint8_t *ip = base + k * stride;
		ip[0] = 0x60;
		ip[1] = 0;
		ip[2] = 0;
		ip[3] = 0;
		ip[4] = (uint8_t)((len - 40) >> 8);
		ip[5] = (uint8_t)(len - 40);
		ip[6] = (uint8_t)nh;
		if (fo >= 0 && 40 + fo + 2 <= (int)len) {
			ip[40 + fo] = 0;
			ip[40 + fo + 1] = 0;
		}
	}
}

hipError_t launch_synth_stamp6(uint8_t *base, uint64_t n, uint64_t stride, uint32_t len, uint32_t nh, int num_cus,
			       hipStream_t st)
{
	uint64_t want = (n + 255) / 256;
	int blocks = (int)(want < (uint64_t)num_cus * 8 ? want : (uint64_t)num_cus * 8);
	if (blocks < 1)
		blocks = 1;
	hipLaunchKernelGGL(synth_stamp6_strided_kernel, dim3(blocks), dim3(256), 0, st, base, n, stride, len, nh);
	return hipGetLastError();
}

__constant__ uint16_t c_imix_len[12] = {64, 576, 64, 64, 576, 64, 1500, 64, 576, 64, 64, 576};
__constant__ uint16_t c_imix_off[12] = {0, 64, 640, 704, 768, 1344, 1408, 2908, 2972, 3548, 3612, 3676};

__global__ __launch_bounds__(256) void synth_imix_kernel(uint8_t *base, uint32_t *desc, uint64_t n)
{
	for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n;
	     k += (uint64_t)gridDim.x * 256) {
		uint64_t off = (k / 12) * (uint64_t)kImixCycleBytes + c_imix_off[k % 12];
		uint32_t len = c_imix_len[k % 12];
		stamp(base + off, len);
		desc[3 * k + 0] = (uint32_t)off;
		desc[3 * k + 1] = (uint32_t)(off >> 32);
		desc[3 * k + 2] = len << 16; // l3_off 0, ip_len
	}
}

// The IMIX frames in ring slots: frame k (length of the 7:4:1 cycle) at
// k * stride + l3_off, e.g. the netmap layout (2048-byte slots, IPv4 at +14).
__global__ __launch_bounds__(256) void synth_ring_kernel(uint8_t *base, uint32_t *desc, uint64_t n, uint64_t stride,
							 uint32_t l3_off)
{
	for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n;
	     k += (uint64_t)gridDim.x * 256) {
		const uint64_t off = k * stride;
		const uint32_t len = c_imix_len[k % 12];
		stamp(base + off + l3_off, len);
		desc[3 * k + 0] = (uint32_t)off;
		desc[3 * k + 1] = (uint32_t)(off >> 32);
		desc[3 * k + 2] = (len << 16) | l3_off;
	}
}

hipError_t launch_synth_ring(uint8_t *base, uint32_t *desc, uint64_t n, uint64_t stride, uint32_t l3_off, int num_cus,
			     hipStream_t st)
{
	uint64_t want = (n + 255) / 256;
	int blocks = (int)(want < (uint64_t)num_cus * 8 ? want : (uint64_t)num_cus * 8);
	if (blocks < 1)
		blocks = 1;
	hipLaunchKernelGGL(synth_ring_kernel, dim3(blocks), dim3(256), 0, st, base, desc, n, stride, l3_off);
	return hipGetLastError();
}

// The IMIX set stamped as IPv6 (cgck_synth_imix_ip6, cgck_synth_imix_ring_ip6):
// the offsets, lengths and descriptors of the two kernels above (stride 0: the
// packed cycle), each frame stamped as synth_stamp6_strided_kernel stamps one.
__global__ __launch_bounds__(256) void synth_imix6_kernel(uint8_t *base, uint32_t *desc, uint64_t n, uint64_t stride,
							  uint32_t l3_off, uint32_t nh)
{
	const int fo = v6_field(nh);
	for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (uint64_t)gridDim.x * 256) {
		const uint64_t off = stride ? k * stride : (k / 12) * (uint64_t)kImixCycleBytes + c_imix_off[k % 12];
		const uint32_t len = c_imix_len[k % 12];
		uint8_t *ip = base + off + l3_off;
		ip[0] = 0x60;
		ip[1] = 0;
		ip[2] = 0;
		ip[3] = 0;
		ip[4] = (uint8_t)((len - 40) >> 8);
		ip[5] = (uint8_t)(len - 40);
		ip[6] = (uint8_t)nh;
		if (fo >= 0 && 40 + fo + 2 <= (int)len) {
			ip[40 + fo] = 0;
			ip[40 + fo + 1] = 0;
		}
		desc[3 * k + 0] = (uint32_t)off;
		desc[3 * k + 1] = (uint32_t)(off >> 32);
		desc[3 * k + 2] = (len << 16) | l3_off;
	}
}

// stride 0: the packed set (l3_off 0)
hipError_t launch_synth_imix6(uint8_t *base, uint32_t *desc, uint64_t n, uint64_t stride, uint32_t l3_off,
			      uint32_t nh, int num_cus, hipStream_t st)
{
	uint64_t want = (n + 255) / 256;
	int blocks = (int)(want < (uint64_t)num_cus * 8 ? want : (uint64_t)num_cus * 8);
	if (blocks < 1)
		blocks = 1;
	hipLaunchKernelGGL(synth_imix6_kernel, dim3(blocks), dim3(256), 0, st, base, desc, n, stride, l3_off, nh);
	return hipGetLastError();
}

// The dual-stack IMIX set (cgck_synth_imix_dual): the same offsets, lengths and
// descriptors; frame k is IPv6 when k % 5 < 2, else IPv4; its protocol by k % 7
// (0-3 TCP, 4-5 UDP, 6 ICMP / ICMPv6), that protocol's checksum field zeroed
// when the frame holds it.
__global__ __launch_bounds__(256) void synth_dual_kernel(uint8_t *base, uint32_t *desc, uint64_t n, uint64_t stride,
							 uint32_t l3_off)
{
	for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (uint64_t)gridDim.x * 256) {
		const uint64_t off = stride ? k * stride : (k / 12) * (uint64_t)kImixCycleBytes + c_imix_off[k % 12];
		const uint32_t len = c_imix_len[k % 12];
		const bool v6 = k % 5 < 2;
		const uint32_t pk = (uint32_t)(k % 7);
		const uint32_t proto = pk < 4 ? 6u : pk < 6 ? 17u : v6 ? 58u : 1u;
		uint8_t *ip = base + off + l3_off;
		int field; // the L4 checksum field from the first header byte
		if (v6) {
			ip[0] = 0x60;
			ip[1] = 0;
			ip[2] = 0;
			ip[3] = 0;
			ip[4] = (uint8_t)((len - 40) >> 8);
			ip[5] = (uint8_t)(len - 40);
			ip[6] = (uint8_t)proto;
			field = 40 + v6_field(proto);
		} else {
			ip[0] = 0x45;
			ip[1] = 0;
			ip[2] = (uint8_t)(len >> 8);
			ip[3] = (uint8_t)len;
			ip[9] = (uint8_t)proto;
			ip[10] = 0;
			ip[11] = 0;
			field = 20 + (proto == 6 ? 16 : proto == 17 ? 6 : 2);
		}
		if (field + 2 <= (int)len) {
			ip[field] = 0;
			ip[field + 1] = 0;
		}
		desc[3 * k + 0] = (uint32_t)off;
		desc[3 * k + 1] = (uint32_t)(off >> 32);
		desc[3 * k + 2] = (len << 16) | l3_off;
	}
}

// stride 0: the packed set (l3_off 0)
hipError_t launch_synth_dual(uint8_t *base, uint32_t *desc, uint64_t n, uint64_t stride, uint32_t l3_off, int num_cus,
			     hipStream_t st)
{
	uint64_t want = (n + 255) / 256;
	int blocks = (int)(want < (uint64_t)num_cus * 8 ? want : (uint64_t)num_cus * 8);
	if (blocks < 1)
		blocks = 1;
	hipLaunchKernelGGL(synth_dual_kernel, dim3(blocks), dim3(256), 0, st, base, desc, n, stride, l3_off);
	return hipGetLastError();
}

// cgck_synth_eth: Ethernet framing in front of a ring set's IP headers, and the
// transport's descriptors {frame_off, l3_off - h, max(ip_len + h, 60)}.
__global__ __launch_bounds__(256) void synth_eth_check_kernel(const uint32_t *desc, uint64_t n, uint32_t *flag)
{
	bool bad = false;
	for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (uint64_t)gridDim.x * 256)
		bad |= (desc[3 * k + 2] & 0xffffu) < 18;
	if (bad)
		atomicOr(flag, 1u);
}

__global__ __launch_bounds__(256) void synth_eth_kernel(uint8_t *base, const uint32_t *desc, uint32_t *raw, uint64_t n,
							uint32_t vlan_every, uint64_t seed)
{
	for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (uint64_t)gridDim.x * 256) {
		const uint32_t lo = desc[3 * k + 0], hi = desc[3 * k + 1], w2 = desc[3 * k + 2];
		const uint32_t l3 = w2 & 0xffffu, len = w2 >> 16;
		const bool t = vlan_every && k % vlan_every == 0;
		const uint32_t h = t ? 18 : 14;
		uint8_t *ip = base + (((uint64_t)hi << 32) | lo) + l3;
		uint8_t *e = ip - h;
		const uint64_t m0 = splitmix64(seed, 2 * k), m1 = splitmix64(seed, 2 * k + 1);
		for (int i = 0; i < 8; ++i)
			e[i] = (uint8_t)(m0 >> (8 * i));
		for (int i = 0; i < 4; ++i)
			e[8 + i] = (uint8_t)(m1 >> (8 * i));
		e[0] &= 0xfe;
		if (t) {
			e[12] = 0x81;
			e[13] = 0x00;
			e[14] = (uint8_t)((k >> 8) & 0x0f);
			e[15] = (uint8_t)k;
		}
		const uint32_t v = ip[0] >> 4;
		const uint32_t et = v == 4 ? 0x0800u : v == 6 ? 0x86DDu : 0x0806u;
		e[h - 2] = (uint8_t)(et >> 8);
		e[h - 1] = (uint8_t)et;
		const uint32_t L = len + h < 60 ? 60 : len + h > 65535 ? 65535 : len + h;
		raw[3 * k + 0] = lo;
		raw[3 * k + 1] = hi;
		raw[3 * k + 2] = (L << 16) | (l3 - h);
	}
}

hipError_t launch_synth_eth_check(const uint32_t *desc, uint64_t n, uint32_t *flag, int num_cus, hipStream_t st)
{
	uint64_t want = (n + 255) / 256;
	int blocks = (int)(want < (uint64_t)num_cus * 8 ? want : (uint64_t)num_cus * 8);
	if (blocks < 1)
		blocks = 1;
	hipLaunchKernelGGL(synth_eth_check_kernel, dim3(blocks), dim3(256), 0, st, desc, n, flag);
	return hipGetLastError();
}

hipError_t launch_synth_eth(uint8_t *base, const uint32_t *desc, uint32_t *raw, uint64_t n, uint32_t vlan_every,
			    uint64_t seed, int num_cus, hipStream_t st)
{
	uint64_t want = (n + 255) / 256;
	int blocks = (int)(want < (uint64_t)num_cus * 8 ? want : (uint64_t)num_cus * 8);
	if (blocks < 1)
		blocks = 1;
	hipLaunchKernelGGL(synth_eth_kernel, dim3(blocks), dim3(256), 0, st, base, desc, raw, n, vlan_every, seed);
	return hipGetLastError();
}

hipError_t launch_synth_fill(uint8_t *base, uint64_t nbytes, uint64_t seed, int num_cus, hipStream_t st)
{
	uint64_t want = (nbytes / 16 + 255) / 256;
	int blocks = (int)(want < (uint64_t)num_cus * 8 ? want : (uint64_t)num_cus * 8);
	if (blocks < 1)
		blocks = 1;
	hipLaunchKernelGGL(synth_fill_kernel, dim3(blocks), dim3(256), 0, st, base, nbytes, seed);
	return hipGetLastError();
}

hipError_t launch_synth_stamp(uint8_t *base, uint64_t n, uint64_t stride, uint32_t len, int num_cus,
			      hipStream_t st)
{
	uint64_t want = (n + 255) / 256;
	int blocks = (int)(want < (uint64_t)num_cus * 8 ? want : (uint64_t)num_cus * 8);
	if (blocks < 1)
		blocks = 1;
	hipLaunchKernelGGL(synth_stamp_strided_kernel, dim3(blocks), dim3(256), 0, st, base, n, stride, len);
	return hipGetLastError();
}

hipError_t launch_synth_imix(uint8_t *base, uint32_t *desc, uint64_t n, int num_cus, hipStream_t st)
{
	uint64_t want = (n + 255) / 256;
	int blocks = (int)(want < (uint64_t)num_cus * 8 ? want : (uint64_t)num_cus * 8);
	if (blocks < 1)
		blocks = 1;
	hipLaunchKernelGGL(synth_imix_kernel, dim3(blocks), dim3(256), 0, st, base, desc, n);
	return hipGetLastError();
}

} // namespace cgck
