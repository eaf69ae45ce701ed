// gple_parse.hip — the doubles of device-resident "%g" text (gple_parse_g): the inverse of gple_format.hip, in the same three launches.
//   parse_count_kernel    every workgroup takes PARSE_CHUNK bytes, 16 per thread, counts the token starts among them and sums up its lines
//   parse_offsets_kernel  one workgroup scans the chunk totals in index order: 64-bit token offsets, the text's token and line counts behind them
//   parse_convert_kernel  every workgroup finds its token starts again, compacts them in LDS and converts them (gple_d2.h), a token per thread and
//                         round: token i of the text in file order goes to values[i]
// A blank is ' ', \t, \n, \v, \f or \r; a token starts at a non-blank byte whose predecessor is blank or which is byte 0, and ends before the next
// blank wherever that is: the conversion reads on into the next chunk.  Chunks are cut in the address space, not in the text: a chunk is 4096 bytes
// from a 4096-byte boundary of the 16-byte piece that holds the text's first byte, so that every piece but the text's first and last is one aligned
// 16-byte load whatever the text pointer is; those two are read byte by byte.
// A line counts when it holds a token start.  What a stretch of text says about lines is (nl, head, tail, full): whether it holds a '\n', whether
// there is a token before its first '\n' and after its last one, and the number of its other '\n' that end a line with a token; two neighbours
// combine associatively (join_lines), threads into a chunk, chunks into runs, runs into the text.
// Offsets come from sums of integers.  The one atomic is an integer minimum, the byte offset of the first malformed token, which does not depend
// on the order: two calls give the same bits.
#include "gple_d2.h"
#include "gple_kernels.h"
#include "gple_scan.h"

namespace gple
{
	namespace
	{
		constexpr int PARSE_THREADS = 256, PIECE = 16;
		constexpr int PARSE_SCAN_THREADS = 1024;
		static_assert(PARSE_THREADS * PIECE == PARSE_CHUNK, "a workgroup's share");

		struct Lines
		{
			unsigned nl, head, tail; // 0 or 1; without a '\n' head = tail = "holds a token start"
			u64 full;
		};
		__host__ __device__ inline Lines join_lines(const Lines& a, const Lines& b)
		{
			if (!b.nl) return Lines{a.nl, a.nl ? a.head : (a.head | b.head), a.tail | b.tail, a.full};
			if (!a.nl) return Lines{1, a.head | b.head, b.tail, b.full};
			return Lines{1, a.head, b.tail, a.full + b.full + (a.tail | b.head)};
		}
		__host__ __device__ inline u64 line_count(const Lines& l) { return l.nl ? l.head + l.full + l.tail : l.head; }
		__host__ __device__ inline unsigned pack_flags(const Lines& l) { return l.nl | (l.head << 1) | (l.tail << 2); }
		__host__ __device__ inline Lines unpack(unsigned flags, u64 full) { return Lines{flags & 1, (flags >> 1) & 1, (flags >> 2) & 1, full}; }

		struct Span
		{
			const unsigned char* text;
			u64 length;
			unsigned skew; // the text pointer's offset from a 16-byte boundary: position a of the aligned space is byte a - skew of the text
		};

		// what a thread knows about its piece: bit b of `starts` = a token starts at byte b; the lines of the piece
		struct Piece
		{
			unsigned starts, tokens;
			Lines lines;
		};
		__device__ inline Piece scan_piece(const Span& S, u64 a0)
		{
			const u64 end = S.skew + S.length; // the text is [skew, end) of the aligned space
			u64 lo = 0x2020202020202020ull, hi = lo; // bytes outside the text read as blanks
			unsigned before = ' ';
			if (a0 >= S.skew && a0 + PIECE <= end)
			{
				const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(S.text + (a0 - S.skew));
				lo = v.x, hi = v.y;
			}
			else
				for (int b = 0; b < PIECE; ++b)
					if (a0 + b >= S.skew && a0 + b < end)
					{
						const u64 c = S.text[a0 + b - S.skew];
						if (b < 8) lo = (lo & ~(0xffull << (8 * b))) | (c << (8 * b));
						else hi = (hi & ~(0xffull << (8 * (b - 8)))) | (c << (8 * (b - 8)));
					}
			if (a0 > S.skew && a0 <= end) before = S.text[a0 - S.skew - 1];
			Piece p{0, 0, Lines{0, 0, 0, 0}};
			bool blank_before = gple_d2::is_blank(before);
			unsigned open = 0; // a token start since the last '\n'
#pragma unroll
			for (int b = 0; b < PIECE; ++b)
			{
				const unsigned c = static_cast<unsigned>((b < 8 ? lo >> (8 * b) : hi >> (8 * (b - 8))) & 0xff);
				const bool blank = gple_d2::is_blank(c);
				if (!blank && blank_before) p.starts |= 1u << b, ++p.tokens, open = 1;
				if (c == '\n')
				{
					if (!p.lines.nl) p.lines.nl = 1, p.lines.head = open;
					else p.lines.full += open;
					open = 0;
				}
				blank_before = blank;
			}
			p.lines.tail = open;
			if (!p.lines.nl) p.lines.head = open;
			return p;
		}

		// sums[c] = (token starts, line flags, full lines) of chunk c
		__global__ __launch_bounds__(PARSE_THREADS) void parse_count_kernel(Span S, uint4* __restrict__ sums)
		{
			__shared__ u64 wave_sums[PARSE_THREADS / 64];
			__shared__ unsigned packed[PARSE_THREADS]; // flags, and the piece's full lines (at most 15) from bit 8 on
			const Piece p = scan_piece(S, static_cast<u64>(blockIdx.x) * PARSE_CHUNK + threadIdx.x * PIECE);
			packed[threadIdx.x] = pack_flags(p.lines) | (static_cast<unsigned>(p.lines.full) << 8);
			u64 total;
			block_exclusive_scan<PARSE_THREADS>(p.tokens, wave_sums, &total); // its barriers publish `packed`
			if (threadIdx.x == 0)
			{
				Lines l = unpack(packed[0], packed[0] >> 8);
				for (int t = 1; t < PARSE_THREADS; ++t) l = join_lines(l, unpack(packed[t], packed[t] >> 8));
				sums[blockIdx.x] = make_uint4(static_cast<unsigned>(total), pack_flags(l), static_cast<unsigned>(l.full), 0);
			}
		}

		// offsets[c] = token starts before chunk c; result = (tokens, lines, no malformed token yet); thread t takes the t-th run of consecutive chunks
		__global__ __launch_bounds__(PARSE_SCAN_THREADS) void parse_offsets_kernel(const uint4* __restrict__ sums, u64 chunks, u64* __restrict__ offsets,
			u64* __restrict__ result)
		{
			__shared__ u64 wave_sums[PARSE_SCAN_THREADS / 64];
			__shared__ u64 run_full[PARSE_SCAN_THREADS];
			__shared__ unsigned run_flags[PARSE_SCAN_THREADS];
			const u64 run = (chunks + PARSE_SCAN_THREADS - 1) / PARSE_SCAN_THREADS;
			const u64 c0 = min(chunks, threadIdx.x * run), c1 = min(chunks, c0 + run);
			u64 mine = 0;
			Lines l{0, 0, 0, 0};
			for (u64 c = c0; c < c1; ++c)
			{
				const uint4 s = sums[c];
				mine += s.x;
				l = join_lines(l, unpack(s.y, s.z));
			}
			run_flags[threadIdx.x] = pack_flags(l), run_full[threadIdx.x] = l.full;
			u64 total;
			u64 at = block_exclusive_scan<PARSE_SCAN_THREADS>(mine, wave_sums, &total);
			for (u64 c = c0; c < c1; ++c)
			{
				offsets[c] = at;
				at += sums[c].x;
			}
			if (threadIdx.x == 0)
			{
				Lines all = unpack(run_flags[0], run_full[0]);
				for (int t = 1; t < PARSE_SCAN_THREADS; ++t) all = join_lines(all, unpack(run_flags[t], run_full[t]));
				result[0] = total, result[1] = line_count(all), result[2] = ~0ull;
			}
		}

		// values[offsets[c] + t] = the t-th token of chunk c, unless the text holds more than `capacity` tokens (then nothing is written)
		__global__ __launch_bounds__(PARSE_THREADS) void parse_convert_kernel(Span S, const uint64_t* __restrict__ table, const u64* __restrict__ offsets,
			u64* result, u64* __restrict__ values, u64 capacity)
		{
			__shared__ u64 wave_sums[PARSE_THREADS / 64];
			__shared__ unsigned short start_at[PARSE_CHUNK / 2]; // a token and its blank: two bytes at least
			if (result[0] > capacity) return;
			const u64 chunk_at = static_cast<u64>(blockIdx.x) * PARSE_CHUNK;
			const Piece p = scan_piece(S, chunk_at + threadIdx.x * PIECE);
			u64 total;
			unsigned slot = static_cast<unsigned>(block_exclusive_scan<PARSE_THREADS>(p.tokens, wave_sums, &total));
#pragma unroll
			for (int b = 0; b < PIECE; ++b)
				if (p.starts >> b & 1) start_at[slot++] = static_cast<unsigned short>(threadIdx.x * PIECE + b);
			__syncthreads();
			const u64 first = offsets[blockIdx.x];
			for (unsigned t = threadIdx.x; t < total; t += PARSE_THREADS)
			{
				const u64 o = chunk_at + start_at[t] - S.skew;
				const unsigned char* const tok = S.text + o;
				int n = 0; // MAX_TOKEN + 1: too long, wherever it ends
				while (n <= gple_d2::MAX_TOKEN && o + n < S.length && !gple_d2::is_blank(tok[n])) ++n;
				uint64_t bits;
				if (gple_d2::parse(tok, n, table, &bits)) values[first + t] = bits;
				else atomicMin(&result[2], o);
			}
		}
	} // namespace

	static size_t parse_chunks(const void* text, size_t length) { return ((reinterpret_cast<uintptr_t>(text) & 15) + length + PARSE_CHUNK - 1) / PARSE_CHUNK; }

	size_t parse_work_bytes(const void* text, size_t length)
	{
		const size_t chunks = parse_chunks(text, length);
		return chunks * sizeof(uint4) + (chunks + 3) * sizeof(u64);
	}

	hipError_t launch_parse(hipStream_t s, const char* text, size_t length, const unsigned long long* table, void* work, double* values, size_t capacity,
		const unsigned long long** result)
	{
		const size_t chunks = parse_chunks(text, length);
		// work (16-byte aligned): the chunk sums, the offsets, the result
		uint4* sums = static_cast<uint4*>(work);
		u64* offsets = reinterpret_cast<u64*>(sums + chunks);
		u64* res = offsets + chunks;
		const Span S{reinterpret_cast<const unsigned char*>(text), length, static_cast<unsigned>(reinterpret_cast<uintptr_t>(text) & 15)};
		const dim3 grid(static_cast<unsigned>(chunks));
		hipLaunchKernelGGL(parse_count_kernel, grid, dim3(PARSE_THREADS), 0, s, S, sums);
		hipLaunchKernelGGL(parse_offsets_kernel, dim3(1), dim3(PARSE_SCAN_THREADS), 0, s, sums, static_cast<u64>(chunks), offsets, res);
		if (values)
			hipLaunchKernelGGL(parse_convert_kernel, grid, dim3(PARSE_THREADS), 0, s, S, reinterpret_cast<const uint64_t*>(table), offsets, res,
				reinterpret_cast<u64*>(values), static_cast<u64>(capacity));
		*result = res;
		return hipGetLastError();
	}
} // namespace gple
