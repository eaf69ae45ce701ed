// gple_d2.h — decimal text to the correctly rounded double: the inverse of gple_g6.h, with the same rules.  One source for the
// host and the device, integers only, no libm, no strtod, no floating-point operation: the result is a bit pattern.  It uses the powers of five
// of gple_g6::build_table.
//
//   token   [+-] digits [. digits] [(e|E) [+-] digits], at least one mantissa digit; or [+-] inf | infinity | nan in any letter case
//   value   D 10^k: D the significant digits without leading and trailing zeros (at most 19: D < 10^19 < 2^64; a 20th non-zero digit makes the
//           token malformed), k the exponent field (saturating) corrected by the position of the point and the zeros left out
//   k >= 0  N = D 5^k, one word times a multi-word integer; the result is the leading 53 bits of N 2^k, rounded half to even on the bit below
//           and the OR of all bits below that
//   k <  0  j = -k: F = floor(D 2^s / 5^j) with s chosen so that F has the 53 bits and at least one more (54 or 55 bits; fewer where the unit
//           stops at 2^-1075, half the least subnormal).  A candidate from the row's reciprocal word is corrected until
//           F 5^j <= D 2^s < (F + 1) 5^j holds in exact multi-word arithmetic (gple_g6::compare), which also says whether the remainder is 0.  The
//           bits of F below the 53 are the half bit and part of the sticky bits; the remainder is the rest of them.
// Whatever the candidate was, the result satisfies the inequalities that define the correctly rounded value.
#pragma once
#include "gple_g6.h"

namespace gple_d2
{
	constexpr int MAX_TOKEN = 64;    // bytes of a token; a longer run of non-blank bytes is malformed
	constexpr int MAX_DIGITS = 19;   // significant digits between the leading and the trailing zeros
	constexpr int K_INF = 308;       // D 10^k with D >= 1 and k > 308 is beyond the largest double
	constexpr int K_ZERO = -343;     // 10^19 10^-344 < 2^-1075: D 10^k with k < -343 rounds to 0
	constexpr int EXP_CAP = 100000;  // the exponent field saturates here: far beyond both cuts, far below int's range with the token's 64 digits added
	constexpr uint64_t INF_BITS = 0x7ff0000000000000ull, NAN_BITS = 0x7ff8000000000000ull, SIGN_BIT = 1ull << 63;
	static_assert(-K_ZERO <= gple_g6::KMAX && K_INF <= gple_g6::KMAX, "the table's rows");

	GPLE_G6_HD inline bool is_blank(unsigned c) { return c == ' ' || (c >= '\t' && c <= '\r'); } // ' ', \t \n \v \f \r

	// mantissa `mant` (at most 2^53, with `round` the bit below it and `sticky` the OR of all bits below that) in units of 2^unit, unit >= -1074;
	// a mantissa below 2^52 comes with unit = -1074 (subnormal)
	GPLE_G6_HD inline uint64_t assemble(uint64_t mant, bool round, bool sticky, int unit)
	{
		if (round && (sticky || (mant & 1))) ++mant;
		if (mant >> 53) mant >>= 1, ++unit;              // 2^53 exactly: carries into the exponent
		if (!(mant >> 52)) return mant;                    // subnormal or 0 (a subnormal that rounds up to 2^52 takes the line below: exponent field 1)
		const int field = unit + 1075;
		return field >= 2047 ? INF_BITS : (static_cast<uint64_t>(field) << 52) | (mant & ((1ull << 52) - 1));
	}

	// the bits of D 10^k, D >= 1, K_ZERO <= k <= K_INF
	GPLE_G6_HD inline uint64_t convert(uint64_t D, int k, const uint64_t* table)
	{
		const int bd = 64 - __builtin_clzll(D);
		if (k >= 0)
		{
			const uint64_t* row = table + static_cast<long>(k) * gple_g6::STRIDE;
			const int bp = gple_g6::pow5_bits(k), nw = (bp + 63) >> 6;
			// N = D 5^k has bd + bp bits or one fewer; G = its bits [top - 64, top) with top = bd + bp, `low` = the OR of the bits below
			const int r = bd + bp - 64;
			uint64_t G = 0, low = 0;
			if (r <= 0) G = (D * row[0]) << -r; // N fits one word
			else
			{
				const int j = r >> 6, c = r & 63;
				uint64_t carry = 0;
				for (int i = 0; i <= nw; ++i)
				{
					uint64_t hi, w = gple_g6::mul64(D, i < nw ? row[i] : 0, &hi);
					w += carry;
					carry = hi + (w < carry);
					if (i < j) low |= w;
					else if (i == j)
					{
						if (c) low |= w & ((1ull << c) - 1);
						G = w >> c;
					}
					else if (i == j + 1 && c)
						G |= w << (64 - c);
				}
			}
			int top = bd + bp;
			if (!(G >> 63)) G <<= 1, --top; // the one fewer: 63 bits of N are still in G, the 53 and the half bit among them
			// N 2^k = (G >> 11) 2^(top - 53 + k) and below
			return assemble(G >> 11, (G >> 10) & 1, (G & 0x3ff) | low, top - 53 + k);
		}
		const int j = -k;
		const uint64_t* row = table + static_cast<long>(j) * gple_g6::STRIDE;
		const int bp = gple_g6::pow5_bits(j), nw = (bp + 63) >> 6;
		// 2^(e - 1) < D 10^k < 2^(e + 1) with e = (bd - 1) - j - (bp - 1): in units of 2^u, u = e - 54, the floor has 54 or 55 bits; the unit
		// does not go below 2^-1075
		const int e = bd - j - bp;
		const int u = e - 54 > -1075 ? e - 54 : -1075;
		// D is used with its leading bit at 2^63 (M = D 2^(64 - bd)), so that the candidate below has 64 good bits however short D is:
		// F = floor(M 2^s / 5^j), s = bp - 10 >= -7 where the unit is not held at 2^-1075, and at most 1075 - 307 where it is
		const uint64_t M = D << (64 - bd);
		const int s = -u - j - (64 - bd);
		// candidate: 5^j = top 2^(bp - 64) (1 + eps) and Q = floor(M R / 2^64) is about M 2^63 / top, so the floor is about Q 2^(s - bp + 1);
		// bp - 1 - s >= 9, so that the few units Q may be off by leave the candidate within one of the floor
		uint64_t Q;
		(void)gple_g6::mul64(M, row[gple_g6::PWORDS], &Q);
		const int sh = bp - 1 - s;
		uint64_t F = sh >= 64 ? 0 : Q >> sh; // below 2^55, so (F + 1) 2^7 stays inside compare's word
		bool rest = true;
		for (int it = 0; it < 6; ++it)
		{
			const int c0 = gple_g6::compare(F, row, nw, M, s); // F 5^j against M 2^s
			if (c0 > 0)
			{
				--F;
				continue;
			}
			if (c0 == 0)
			{
				rest = false;
				break;
			}
			if (gple_g6::compare(F + 1, row, nw, M, s) > 0) break; // below F + 1 and not F: a remainder
			++F;
		}
		const int bf = F ? 64 - __builtin_clzll(F) : 0;
		const int drop = bf - 53 > 1 ? bf - 53 : 1; // 1 or 2; the unit u + drop is max(E - 52, -1074)
		return assemble(F >> drop, (F >> (drop - 1)) & 1, (F & ((1ull << (drop - 1)) - 1)) || rest, u + drop);
	}

	GPLE_G6_HD inline unsigned lower(unsigned c) { return c >= 'A' && c <= 'Z' ? c + 32 : c; }

	// letters of s[i .. n) against a lower-case word of `len` letters packed eight bits each, first letter lowest
	GPLE_G6_HD inline bool is_word(const unsigned char* s, int i, int n, uint64_t word, int len)
	{
		if (n - i != len) return false;
		for (int b = 0; b < len; ++b)
			if (lower(s[i + b]) != ((word >> (8 * b)) & 0xff)) return false;
		return true;
	}

	// the token s[0 .. n) (no blanks inside) -> *bits, the correctly rounded double's bit pattern; false: malformed (n outside 1 .. MAX_TOKEN,
	// not of the grammar, or more than MAX_DIGITS significant digits), *bits untouched
	GPLE_G6_HD inline bool parse(const unsigned char* s, int n, const uint64_t* table, uint64_t* bits)
	{
		if (n < 1 || n > MAX_TOKEN) return false;
		int i = 0;
		uint64_t sign = 0;
		if (s[0] == '+' || s[0] == '-') sign = s[0] == '-' ? SIGN_BIT : 0, i = 1;
		if (i < n && (lower(s[i]) == 'i' || lower(s[i]) == 'n'))
		{
			if (is_word(s, i, n, 0x666e69ull, 3) || is_word(s, i, n, 0x7974696e69666e69ull, 8)) // "inf", "infinity"
			{
				*bits = sign | INF_BITS;
				return true;
			}
			if (!is_word(s, i, n, 0x6e616eull, 3)) return false; // "nan"
			*bits = NAN_BITS;
			return true;
		}
		uint64_t D = 0;
		int k = 0, nd = 0, zeros = 0; // zeros: digits 0 seen after the last digit in D, not yet multiplied in
		bool digits = false, point = false;
		for (; i < n; ++i)
		{
			const unsigned c = s[i];
			if (c == '.')
			{
				if (point) return false;
				point = true;
				continue;
			}
			if (c < '0' || c > '9') break;
			digits = true;
			if (point) --k;
			if (c == '0')
			{
				if (nd) ++zeros; // a leading zero otherwise
				continue;
			}
			if (nd + zeros + 1 > MAX_DIGITS) return false;
			for (int z = 0; z < zeros; ++z) D *= 10;
			D = D * 10 + (c - '0');
			nd += zeros + 1, zeros = 0;
		}
		if (!digits) return false;
		k += zeros; // the trailing zeros stay out of D
		if (i < n)
		{
			if (s[i] != 'e' && s[i] != 'E') return false;
			++i;
			bool minus = false;
			if (i < n && (s[i] == '+' || s[i] == '-')) minus = s[i] == '-', ++i;
			if (i == n) return false;
			int ex = 0;
			for (; i < n; ++i)
			{
				const unsigned c = s[i];
				if (c < '0' || c > '9') return false;
				if (ex < EXP_CAP) ex = ex * 10 + static_cast<int>(c - '0');
			}
			k += minus ? -ex : ex;
		}
		*bits = sign | (D == 0 || k < K_ZERO ? 0 : k > K_INF ? INF_BITS : convert(D, k, table));
		return true;
	}
} // namespace gple_d2
