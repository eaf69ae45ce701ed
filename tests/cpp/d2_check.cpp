// d2_check.cpp — csrc/gple_d2.h against the C library's strtod, bit for bit (tests/test_parse_host.py compiles and runs it; host only).
//   d2_check [random_count [threads]]
// defaults: 10000000 random bit patterns (splitmix64, as g6_check.cpp), as many threads as the machine reports (at most 16).  Families:
//   the "%g", "%.9g", "%.17g" and "%.19g" texts of every random pattern (the "%.17g" text must also give the pattern itself back);
//   near-halfway strings: the midpoint of a double and its successor, cut to 17, 18 and 19 digits, and that number plus one in the last
//     digit — for every tenth random pattern and for 2^e, e = -1074 .. 1023 — and the same cuts of the doubles 2^e themselves;
//   the range edges, 1e-343 .. 1e308 with a short and a 19-digit mantissa, the grammar's corners, the malformed forms (rejected).
// Every string is compared together with its negative.  Prints the number of strings compared and of mismatches (the first few in full); exit
// status 1 if any.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../gaussian_process_liouville_equation_amd/csrc/gple_d2.h"

static std::vector<uint64_t> table(gple_g6::TABLE_WORDS);

static bool header(const std::string& s, uint64_t* bits)
{
	return gple_d2::parse(reinterpret_cast<const unsigned char*>(s.data()), static_cast<int>(s.size()), table.data(), bits);
}

struct Tally
{
	unsigned long long compared = 0, mismatches = 0;
	void fail(const char* what, const std::string& s, uint64_t got, uint64_t want)
	{
		if (mismatches++ < 8) std::printf("MISMATCH (%s) '%s': header %016llx, expected %016llx\n", what, s.c_str(), (unsigned long long)got, (unsigned long long)want);
	}
	// s against strtod; returns the header's bits
	uint64_t one(const std::string& s)
	{
		char* end = nullptr;
		const double w = std::strtod(s.c_str(), &end);
		uint64_t want, got = 0x5555555555555555ull;
		std::memcpy(&want, &w, 8);
		if (std::isnan(w)) want = gple_d2::NAN_BITS; // one quiet NaN whatever the sign
		++compared;
		if (*end || !header(s, &got) || got != want) fail("strtod", s, got, want);
		return got;
	}
	uint64_t both(const std::string& s)
	{
		const uint64_t r = one(s);
		one((s[0] == '-' ? "" : "-") + (s[0] == '-' || s[0] == '+' ? s.substr(1) : s));
		return r;
	}
	void rejected(const std::string& s)
	{
		for (const std::string& t : {s, "-" + s})
		{
			uint64_t got = 0x5555555555555555ull;
			++compared;
			if (header(t, &got) || got != 0x5555555555555555ull) fail("must be rejected", t, got, 0);
		}
	}
	// the decimal expansion `full` ("d.ddd...e+XX" with at least 19 digits) cut to 17, 18 and 19 digits, each also with one more in the last digit
	void cuts(const char* full)
	{
		const char* ex = std::strchr(full, 'e');
		std::string digits(1, full[0]);
		digits.append(full + 2, ex);
		for (int nd = 17; nd <= 19; ++nd)
			for (int up = 0; up < 2; ++up)
			{
				std::string d = digits.substr(0, nd);
				if (up)
				{
					int i = nd - 1;
					while (i >= 0 && d[i] == '9') d[i--] = '0';
					if (i >= 0) ++d[i];
					else d = "1" + d; // 999...9 + 1: one digit more, a trailing zero
				}
				const int shift = static_cast<int>(d.size()) - nd;
				both(d.substr(0, 1) + "." + d.substr(1) + "e" + std::to_string(std::atoi(ex + 1) + shift));
			}
	}
	// around v > 0: the double's own expansion and the midpoint to its successor (exact in long double: 54 bits)
	void near_half(double v)
	{
		char text[96];
		const double next = std::nextafter(v, INFINITY);
		if (!std::isfinite(next)) return;
		std::snprintf(text, sizeof text, "%.40Le", (static_cast<long double>(v) + static_cast<long double>(next)) / 2);
		cuts(text);
	}
};

static uint64_t splitmix64(uint64_t s0, uint64_t n)
{
	uint64_t z = s0 + (n + 1) * 0x9e3779b97f4a7c15ull;
	z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
	z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
	return z ^ (z >> 31);
}

int main(int argc, char** argv)
{
	static_assert(sizeof(long double) >= 10 && __LDBL_MANT_DIG__ >= 64, "the midpoints need 54 bits and the double's exponent range");
	const long random_count = argc > 1 ? std::atol(argv[1]) : 10000000;
	const int threads = std::max(1, argc > 2 ? std::atoi(argv[2]) : std::min(16, static_cast<int>(std::thread::hardware_concurrency())));
	gple_g6::build_table(table.data());
	std::vector<Tally> tally(threads);
	std::vector<std::thread> pool;
	for (int w = 0; w < threads; ++w)
		pool.emplace_back([&, w] {
			Tally& t = tally[w];
			char text[96];
			for (long i = random_count * w / threads; i < random_count * (w + 1) / threads; ++i)
			{
				const uint64_t b = splitmix64(20240607, i);
				double v;
				std::memcpy(&v, &b, sizeof v);
				for (const char* f : {"%g", "%.9g", "%.19g"})
				{
					std::snprintf(text, sizeof text, f, v);
					t.both(text);
				}
				std::snprintf(text, sizeof text, "%.17g", v);
				const uint64_t back = t.both(text);
				if (std::isfinite(v) && back != b) t.fail("%.17g gives the value back", text, back, b);
				if (i % 10 == 0 && std::isfinite(v)) t.near_half(std::fabs(v));
			}
			if (w) return;
			for (int e = -1074; e <= 1023; ++e)
			{
				const double v = std::ldexp(1.0, e);
				std::snprintf(text, sizeof text, "%.40e", v);
				t.cuts(text);
				t.near_half(v);
				t.near_half(std::nextafter(v, 0.0)); // the midpoint below 2^e
			}
			// the range edges
			for (const char* s : {"4.9e-324", "2.4703282292062327e-324", "2.4703282292062328e-324", "2.2250738585072011e-308", "2.2250738585072014e-308",
					 "1.7976931348623157e308", "1.797693134862315807e308", "1.797693134862315808e308", "2.470328229206232720e-324", "2.470328229206232721e-324",
					 "1e999999999999", "1e-999999999999", "0e999999999999", "1e309", "1e-344", "9999999999999999999e-343", "9999999999999999999e-344",
					 "0.0000000000000000000000000000000000000000000000000001e360"})
				t.both(s);
			for (int k = -343; k <= 308; ++k)
			{
				t.both("1e" + std::to_string(k));
				t.both("1.234567890123456789e" + std::to_string(k));
				t.both("9999999999999999999e" + std::to_string(k - 18));
				t.both("8.98846567431158e" + std::to_string(k));
			}
			// the grammar
			for (const char* s : {"+1", ".5", "5.", "1E5", "1e+06", "-0", "0", "0.0", "000123.4500e-0007", "1234567890123456789000000000000000000000",
					 "1234567890.123456789000000000000000000000", "0.00000000001234567890123456789000000000000", "1.000000000000000000e-330",
					 "1000000000000000000000e-330", "inf", "INF", "Inf", "infinity", "INFINITY", "Infinity", "+inf", "nan", "NaN", "NAN", "+nan", "00", "0e0", "1e0000000000000000005"})
				t.both(s);
			for (const char* s : {"0x1p3", "0x10", "", "+", ".", "e5", ".e5", "1e", "1e+", "1e-", "1a", "a1", "1.2.3", "1e5.5", "1e5e5", "1+1", "--1", "+-1", "in", "infi",
					 "infinit", "infinityy", "na", "nana", "nan(1)", "1f", "1d5", "1,5", "12345678901234567891", "1.2345678901234567891", "1000000000000000000001",
					 "0.10000000000000000001", "1_000"})
				t.rejected(s);
			t.both(std::string(62, '0') + "1"); // 63 and 64 bytes
			t.rejected(std::string(64, '0') + "1");
		});
	for (std::thread& th : pool) th.join();
	Tally sum;
	for (const Tally& t : tally) sum.compared += t.compared, sum.mismatches += t.mismatches;
	std::printf("compared %llu values, %llu mismatches\n", sum.compared, sum.mismatches);
	return sum.mismatches ? 1 : 0;
}
