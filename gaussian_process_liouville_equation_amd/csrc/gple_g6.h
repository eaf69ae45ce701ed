// gple_g6.h — the bytes of C's "%g" (precision 6) of a double, correctly rounded for every double, as plain integer C++ that the host and the
// device compile from this one source.  No libm, no printf, no floating-point arithmetic at all: the value is taken apart into
// m * 2^e and scaled by an exact power of five from a table.
//
//   v * 10^q = m * 5^q * 2^(e+q)            q >= 0: one word times a multi-word integer; the six digits are a bit field of the product and the
//                                                   bits below it say below / exactly / above one half
//   v * 10^q = m * 2^(e-k) / 5^k, k = -q    q <  0: a candidate floor F from a 64-bit reciprocal of the leading word of 5^k, then corrected until
//                                                   F 5^k <= m 2^(e-k) < (F+1) 5^k holds in exact multi-word arithmetic; the half comes from
//                                                   comparing (2F+1) 5^k with m 2^(e-k+1)
//
// Whatever the candidate was, the result satisfies the inequalities that define the correctly rounded value: exactness does not rest on the
// quality of an estimate.  The decade X is estimated from the binary exponent; an estimate off by one shows as a floor outside [10^5, 10^6) of
// the unrounded value and is redone, and a floor that rounds up to 10^6 carries into the next decade.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GPLE_G6_HD __host__ __device__
#else
#define GPLE_G6_HD
#endif

namespace gple_g6
{
	constexpr int KMAX = 343;   // rows 5^0 .. 5^343 (the scales needed are 5^0 .. 5^330)
	constexpr int PWORDS = 13;  // 64-bit words of a power, least significant first (5^343 has 797 bits)
	constexpr int STRIDE = 14;  // words of a row: the power, then floor((2^127 - 1) / top) with top = the leading 64 bits of the power, normalised
	constexpr int TABLE_WORDS = (KMAX + 1) * STRIDE;
	constexpr int MAX_BYTES = 13; // "-1.23457e-308"
	constexpr uint64_t TOO_LARGE = 1ull << 62; // what scaled() returns for "at least 10^6", whatever the exact value

	// the table, by repeated multiplication (host)
	inline void build_table(uint64_t* t)
	{
		uint64_t cur[PWORDS] = {1};
		for (int k = 0; k <= KMAX; ++k)
		{
			uint64_t* row = t + static_cast<long>(k) * STRIDE;
			int hw = 0;
			for (int i = 0; i < PWORDS; ++i)
			{
				row[i] = cur[i];
				if (cur[i]) hw = i;
			}
			const int lz = __builtin_clzll(cur[hw]);
			const uint64_t top = lz ? (cur[hw] << lz) | (hw ? cur[hw - 1] >> (64 - lz) : 0) : cur[hw];
			row[PWORDS] = static_cast<uint64_t>(((static_cast<unsigned __int128>(1) << 127) - 1) / top);
			uint64_t carry = 0;
			for (int i = 0; i < PWORDS; ++i)
			{
				const unsigned __int128 p = static_cast<unsigned __int128>(cur[i]) * 5 + carry;
				cur[i] = static_cast<uint64_t>(p);
				carry = static_cast<uint64_t>(p >> 64);
			}
		}
	}

	GPLE_G6_HD inline uint64_t mul64(uint64_t a, uint64_t b, uint64_t* hi)
	{
#if defined(__HIP_DEVICE_COMPILE__)
		*hi = __umul64hi(a, b);
		return a * b;
#else
		const unsigned __int128 p = static_cast<unsigned __int128>(a) * b;
		*hi = static_cast<uint64_t>(p >> 64);
		return static_cast<uint64_t>(p);
#endif
	}

	// bit length of 5^k (exact for 0 <= k <= 3528) and the words it fills
	GPLE_G6_HD inline int pow5_bits(int k) { return static_cast<int>((static_cast<uint32_t>(k) * 1217359u) >> 19) + 1; }

	// sign of A * 5^k - m * 2^t (t < 0: of A * 5^k * 2^-t - m; the caller keeps A * 2^-t below 2^64), words streamed from the low end
	GPLE_G6_HD inline int compare(uint64_t A, const uint64_t* row, int nw, uint64_t m, int t)
	{
		if (t < 0) A <<= -t, t = 0;
		const int tw = t >> 6, tb = t & 63;
		const int n_it = nw + 1 > tw + 2 ? nw + 1 : tw + 2; // <= 17: nw <= 13, t <= 972
		uint64_t carry = 0, nonzero = 0;
		bool borrow = false;
		for (int i = 0; i < n_it; ++i)
		{
			uint64_t hi, lo = mul64(A, i < nw ? row[i] : 0, &hi);
			lo += carry;
			carry = hi + (lo < carry);
			const uint64_t mi = i == tw ? m << tb : (i == tw + 1 && tb) ? m >> (64 - tb) : 0;
			const uint64_t d = lo - mi - borrow;
			borrow = lo < mi || (lo == mi && borrow);
			nonzero |= d;
		}
		return borrow ? -1 : nonzero ? 1 : 0;
	}

	// F = floor(m 2^e 10^q), and *half = -1 / 0 / +1: the remainder is below / exactly / above one half.  Exact whenever 10^5 <= F < 10^6; a value
	// below 10^5 gives some F < 10^5 and a value of 10^6 or more some F >= 10^6 (the caller then moves the decade and asks again).
	GPLE_G6_HD inline uint64_t scaled(uint64_t m, int e, int q, const uint64_t* table, int* half)
	{
		*half = -1;
		if (q >= 0)
		{
			const uint64_t* row = table + static_cast<long>(q) * STRIDE;
			const int nw = (pow5_bits(q) + 63) >> 6;
			const int r = -(e + q); // the product m 5^q is shifted right by r
			if (r <= 0) return TOO_LARGE; // an integer of at least 2^52 for a normal m; a subnormal m never gets here (e + q < 0)
			// G = bits [r - 1, r + 63) of the product: F and the half bit; `low` = the bits below, `high` = the bits above
			const int j = (r - 1) >> 6, c = (r - 1) & 63;
			uint64_t carry = 0, G = 0, low = 0, high = 0;
			for (int i = 0; i <= nw; ++i)
			{
				uint64_t hi, w = mul64(m, i < nw ? row[i] : 0, &hi);
				w += carry;
				carry = hi + (w < carry);
				if (i < j) low |= w;
				else if (i == j)
				{
					if (c) low |= w & ((1ull << c) - 1);
					G = w >> c;
				}
				else if (i == j + 1 && c)
				{
					G |= w << (64 - c);
					high |= w >> c;
				}
				else
					high |= w;
			}
			if (high || (G >> 40)) return TOO_LARGE;
			*half = (G & 1) ? (low ? 1 : 0) : -1;
			return G >> 1;
		}
		const int k = -q;
		const uint64_t* row = table + static_cast<long>(k) * STRIDE;
		const int bp = pow5_bits(k), nw = (bp + 63) >> 6;
		const int s = e - k; // the value is m 2^s / 5^k
		if (s < -38) return 0; // below 2^53 2^-38 = 2^15 < 10^5
		// candidate: 5^k = top 2^(bp - 64) (1 + eps), 0 <= eps < 2^-63, and m 2^64 / top - 3 < Q <= m 2^64 / top, so the floor is within one of
		// Q >> (bp - s); the loop below does not depend on that
		uint64_t qh, ql = mul64(m, row[PWORDS], &qh);
		const uint64_t Q = (qh << 1) | (ql >> 63);
		const int sh = bp - s;
		if (sh < 0) return TOO_LARGE; // m 2^s >= 2^bp > 5^k ... and far more: at least 2^52 times it
		uint64_t F = sh >= 64 ? 0 : Q >> sh;
		if (F > (1ull << 21)) return TOO_LARGE; // the floor is at least F - 1 >= 2^21 > 10^6
		// (2F + 1) 2^(-s-1) and (F + 1) 2^-s stay below 2^22 2^38 = 2^60
		for (int it = 0; it < 4; ++it)
		{
			const int c1 = compare(2 * F + 1, row, nw, m, s + 1); // (2F + 1) 5^k against 2 m 2^s
			if (c1 <= 0)
			{
				// at or above F + 1/2, so F 5^k <= m 2^s; is it below F + 1?
				if (compare(F + 1, row, nw, m, s) <= 0)
				{
					++F;
					continue;
				}
				*half = c1 < 0 ? 1 : 0;
				return F;
			}
			// below F + 1/2, so below F + 1; is it at least F?
			if (compare(F, row, nw, m, s) > 0)
			{
				--F;
				continue;
			}
			*half = -1;
			return F;
		}
		return F; // not reached: the candidate is within one of the floor
	}

	// up to 16 bytes held in two registers (no addressable buffer: device code keeps it out of scratch memory)
	struct Text
	{
		uint64_t lo = 0, hi = 0;
		int n = 0;
		GPLE_G6_HD void push(unsigned ch)
		{
			if (n < 8) lo |= static_cast<uint64_t>(ch) << (8 * n);
			else hi |= static_cast<uint64_t>(ch) << (8 * (n - 8));
			++n;
		}
		GPLE_G6_HD unsigned at(int i) const { return static_cast<unsigned>((i < 8 ? lo >> (8 * i) : hi >> (8 * (i - 8))) & 0xff); }
	};

	// appends "%g" of v to t (at most MAX_BYTES bytes)
	GPLE_G6_HD inline void append(Text& t, double v, const uint64_t* table)
	{
		const uint64_t bits = __builtin_bit_cast(uint64_t, v);
		const bool neg = bits >> 63;
		const int ex = static_cast<int>((bits >> 52) & 0x7ff);
		const uint64_t frac = bits & ((1ull << 52) - 1);
		if (ex == 0x7ff)
		{
			if (frac) t.push('n'), t.push('a'), t.push('n'); // no sign, as Python's "%g" % v
			else
			{
				if (neg) t.push('-');
				t.push('i'), t.push('n'), t.push('f');
			}
			return;
		}
		if (neg) t.push('-');
		if (ex == 0 && frac == 0)
		{
			t.push('0');
			return;
		}
		const uint64_t m = ex ? frac | (1ull << 52) : frac;
		const int e = ex ? ex - 1075 : -1074;
		const int e2 = e + 63 - __builtin_clzll(m); // 2^e2 <= v < 2^(e2 + 1)
		int X = (e2 * 78913) >> 18;                  // floor(e2 log10 2) for |e2| <= 1650: the decade of 2^e2, at most one below that of v
		uint64_t F = 0;
		int half = -1;
		for (int attempt = 0; attempt < 3; ++attempt)
		{
			F = scaled(m, e, 5 - X, table, &half);
			if (F < 100000) --X;
			else if (F >= 1000000) ++X;
			else break;
		}
		uint32_t D = static_cast<uint32_t>(F) + ((half > 0 || (half == 0 && (F & 1))) ? 1u : 0u);
		if (D == 1000000) D = 100000, ++X; // 9.999995 and above: into the next decade
		int nd = 6;                        // significant digits without the trailing zeros
		for (uint32_t z = D; nd > 1 && z % 10 == 0; z /= 10) --nd;
		uint32_t rest = D; // the leading digit is rest / 10^5
		auto digit = [&]() {
			const uint32_t d = rest / 100000;
			rest = (rest - d * 100000) * 10;
			t.push('0' + d);
		};
		if (X < -4 || X >= 6)
		{
			digit();
			if (nd > 1) t.push('.');
			for (int i = 1; i < nd; ++i) digit();
			t.push('e');
			t.push(X < 0 ? '-' : '+');
			const uint32_t a = X < 0 ? -X : X;
			if (a >= 100) t.push('0' + a / 100);
			t.push('0' + a / 10 % 10);
			t.push('0' + a % 10);
		}
		else if (X >= 0)
		{
			const int count = nd > X + 1 ? nd : X + 1;
			for (int i = 0; i < count; ++i)
			{
				digit();
				if (i == X && nd > X + 1) t.push('.');
			}
		}
		else
		{
			t.push('0');
			t.push('.');
			for (int i = 0; i < -X - 1; ++i) t.push('0');
			for (int i = 0; i < nd; ++i) digit();
		}
	}

	// "%g" of v into out (at most MAX_BYTES bytes, no terminator); returns the length
	GPLE_G6_HD inline int format(double v, char* out, const uint64_t* table)
	{
		Text t;
		append(t, v, table);
		for (int i = 0; i < t.n; ++i) out[i] = static_cast<char>(t.at(i));
		return t.n;
	}
} // namespace gple_g6
