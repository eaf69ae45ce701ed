// gple_format.hip — the "%g" text of device-resident doubles (gple_format_g).  What the reference's streams write number by number
// (output_phase_space_distribution, general.cpp:384-392; output_phase, output.cpp:180-232) is produced here by three launches:
//   format_sizes_kernel    every workgroup converts its FMT_BLOCK numbers (gple_g6.h) and sums the bytes of its items
//   format_offsets_kernel  one workgroup scans the workgroup totals in index order: 64-bit byte offsets, the text's length behind the last one
//   format_write_kernel    every workgroup scans its own item lengths, lays its bytes out in LDS and stores them in aligned 16-byte pieces
// An item is one number with what surrounds it: the leading blank (none at the start of a line under GPLE_FORMAT_JOIN), then '\n' after the last
// number of a line and a second '\n' after the last line of a block — at most 1 + 13 + 2 = 16 bytes, so an item travels in two registers.
// Offsets come from sums of integers only and nothing is atomic: two calls give the same bytes.  The write kernel either converts again or reads
// the items the size kernel kept (16-byte slots and a length byte per number; `slots` of launch_format).
#include "gple_g6.h"
#include "gple_kernels.h"
#include "gple_scan.h"

namespace gple
{
	namespace
	{
		constexpr int FMT_THREADS = 256, FMT_ITEMS = 4;
		constexpr int SCAN_THREADS = 1024;
		static_assert(FMT_THREADS * FMT_ITEMS == FORMAT_BLOCK, "a workgroup's share");

		struct Layout
		{
			u64 count, per_line, lines_per_block;
			int join;
		};

		// the items of the FMT_ITEMS numbers from g0 on (empty beyond count); returns their bytes
		__device__ inline unsigned convert_items(const double* __restrict__ values, const Layout& L, const uint64_t* __restrict__ table, u64 g0,
			gple_g6::Text (&items)[FMT_ITEMS])
		{
			u64 col = g0 % L.per_line;
			u64 line_in_block = L.lines_per_block ? (g0 / L.per_line) % L.lines_per_block : 0;
			unsigned bytes = 0;
#pragma unroll
			for (int k = 0; k < FMT_ITEMS; ++k)
			{
				gple_g6::Text t;
				if (g0 + k < L.count)
				{
					if (!(L.join && col == 0)) t.push(' ');
					gple_g6::append(t, values[g0 + k], table);
					if (++col == L.per_line)
					{
						col = 0;
						t.push('\n');
						if (L.lines_per_block && ++line_in_block == L.lines_per_block)
						{
							line_in_block = 0;
							t.push('\n');
						}
					}
				}
				items[k] = t;
				bytes += t.n;
			}
			return bytes;
		}

		template <bool SLOTS>
		__global__ __launch_bounds__(FMT_THREADS) void format_sizes_kernel(const double* __restrict__ values, Layout L, const uint64_t* __restrict__ table,
			unsigned* __restrict__ block_bytes, ulonglong2* __restrict__ slots, unsigned char* __restrict__ slot_bytes)
		{
			__shared__ u64 wave_sums[FMT_THREADS / 64];
			const u64 g0 = static_cast<u64>(blockIdx.x) * FORMAT_BLOCK + threadIdx.x * FMT_ITEMS;
			gple_g6::Text items[FMT_ITEMS];
			const unsigned bytes = convert_items(values, L, table, g0, items);
			if (SLOTS)
			{
#pragma unroll
				for (int k = 0; k < FMT_ITEMS; ++k)
					if (g0 + k < L.count)
					{
						slots[g0 + k] = make_ulonglong2(items[k].lo, items[k].hi);
						slot_bytes[g0 + k] = static_cast<unsigned char>(items[k].n);
					}
			}
			u64 total;
			block_exclusive_scan<FMT_THREADS>(bytes, wave_sums, &total);
			if (threadIdx.x == 0) block_bytes[blockIdx.x] = static_cast<unsigned>(total);
		}

		// offsets[b] = sum of block_bytes[0 .. b), offsets[blocks] = the length of the text; thread t takes the t-th run of consecutive workgroups
		__global__ __launch_bounds__(SCAN_THREADS) void format_offsets_kernel(const unsigned* __restrict__ block_bytes, u64 blocks, u64* __restrict__ offsets)
		{
			__shared__ u64 wave_sums[SCAN_THREADS / 64];
			const u64 run = (blocks + SCAN_THREADS - 1) / SCAN_THREADS;
			const u64 b0 = min(blocks, threadIdx.x * run), b1 = min(blocks, b0 + run);
			u64 mine = 0;
			for (u64 b = b0; b < b1; ++b) mine += block_bytes[b];
			u64 total;
			u64 at = block_exclusive_scan<SCAN_THREADS>(mine, wave_sums, &total);
			for (u64 b = b0; b < b1; ++b)
			{
				offsets[b] = at;
				at += block_bytes[b];
			}
			if (threadIdx.x == 0) offsets[blocks] = total;
		}

		template <bool SLOTS>
		__global__ __launch_bounds__(FMT_THREADS) void format_write_kernel(const double* __restrict__ values, Layout L, const uint64_t* __restrict__ table,
			const u64* __restrict__ offsets, const ulonglong2* __restrict__ slots, const unsigned char* __restrict__ slot_bytes, unsigned char* __restrict__ text)
		{
			// the workgroup's bytes as they will lie in memory: stage[0] is the aligned 16-byte piece that holds the workgroup's first byte
			__shared__ uint4 stage[FORMAT_BLOCK + 1];
			__shared__ u64 wave_sums[FMT_THREADS / 64];
			const u64 g0 = static_cast<u64>(blockIdx.x) * FORMAT_BLOCK + threadIdx.x * FMT_ITEMS;
			gple_g6::Text items[FMT_ITEMS];
			unsigned bytes = 0;
			if (SLOTS)
			{
#pragma unroll
				for (int k = 0; k < FMT_ITEMS; ++k)
				{
					items[k] = gple_g6::Text{};
					if (g0 + k < L.count)
					{
						const ulonglong2 s = slots[g0 + k];
						items[k].lo = s.x, items[k].hi = s.y, items[k].n = slot_bytes[g0 + k];
					}
					bytes += items[k].n;
				}
			}
			else
				bytes = convert_items(values, L, table, g0, items);
			u64 total;
			const unsigned first = static_cast<unsigned>(block_exclusive_scan<FMT_THREADS>(bytes, wave_sums, &total));
			const u64 base = offsets[blockIdx.x];
			const unsigned skew = static_cast<unsigned>((reinterpret_cast<uintptr_t>(text) + base) & 15);
			unsigned char* const staged = reinterpret_cast<unsigned char*>(stage);
			unsigned at = skew + first; // < 16 + FORMAT_BLOCK * 16
#pragma unroll
			for (int k = 0; k < FMT_ITEMS; ++k)
				for (int b = 0; b < items[k].n; ++b) staged[at++] = static_cast<unsigned char>(items[k].at(b));
			__syncthreads();
			const unsigned end = skew + static_cast<unsigned>(total);
			unsigned char* const dst = text + base - skew; // 16-byte aligned; only the bytes [skew, end) of it are this workgroup's
			for (unsigned piece = threadIdx.x; piece * 16 < end; piece += FMT_THREADS)
			{
				const unsigned lo = piece * 16, hi = lo + 16;
				if (lo >= skew && hi <= end) reinterpret_cast<uint4*>(dst)[piece] = stage[piece];
				else
					for (unsigned b = max(lo, skew); b < min(hi, end); ++b) dst[b] = staged[b];
			}
		}
	} // namespace

	static size_t format_blocks(size_t count) { return (count + FORMAT_BLOCK - 1) / FORMAT_BLOCK; }

	size_t format_work_bytes(size_t count, bool slots)
	{
		const size_t blocks = format_blocks(count);
		return (blocks + 1) * sizeof(u64) + round_up(blocks * sizeof(unsigned), 16) + (slots ? count * 16 + count : 0);
	}

	hipError_t launch_format(hipStream_t s, const double* values, size_t count, size_t per_line, size_t lines_per_block, bool join,
		const unsigned long long* table, void* work, bool slots, char* text, const unsigned long long** length)
	{
		const size_t blocks = format_blocks(count);
		// work (16-byte aligned): the slots, the offsets, the workgroup totals, the slots' lengths
		unsigned char* w = static_cast<unsigned char*>(work);
		ulonglong2* slot = reinterpret_cast<ulonglong2*>(w);
		if (slots) w += count * 16;
		u64* offsets = reinterpret_cast<u64*>(w);
		w += (blocks + 1) * sizeof(u64);
		unsigned* block_bytes = reinterpret_cast<unsigned*>(w);
		w += round_up(blocks * sizeof(unsigned), 16);
		unsigned char* slot_bytes = w;
		const Layout L{count, per_line, lines_per_block, join ? 1 : 0};
		const uint64_t* tab = reinterpret_cast<const uint64_t*>(table);
		unsigned char* out = reinterpret_cast<unsigned char*>(text);
		const dim3 grid(static_cast<unsigned>(blocks));
		if (slots) hipLaunchKernelGGL(format_sizes_kernel<true>, grid, dim3(FMT_THREADS), 0, s, values, L, tab, block_bytes, slot, slot_bytes);
		else hipLaunchKernelGGL(format_sizes_kernel<false>, grid, dim3(FMT_THREADS), 0, s, values, L, tab, block_bytes, slot, slot_bytes);
		hipLaunchKernelGGL(format_offsets_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, block_bytes, static_cast<u64>(blocks), offsets);
		if (slots) hipLaunchKernelGGL(format_write_kernel<true>, grid, dim3(FMT_THREADS), 0, s, values, L, tab, offsets, slot, slot_bytes, out);
		else hipLaunchKernelGGL(format_write_kernel<false>, grid, dim3(FMT_THREADS), 0, s, values, L, tab, offsets, slot, slot_bytes, out);
		*length = offsets + blocks;
		return hipGetLastError();
	}
} // namespace gple
