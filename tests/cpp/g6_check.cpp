// g6_check.cpp — csrc/gple_g6.h against the C library's "%g" on finite doubles (tests/test_format_host.py compiles and runs it; host only).
//   g6_check [random_count [tie_stride [threads]]]
// defaults: 20000000 random bit patterns, every six-digit prefix D of the tie strings (tie_stride 1), as many threads as the machine reports (at
// most 16).  Every value is compared together with its negative.  Prints the number of values compared and of mismatches (the first few in
// full); exit status 1 if any.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../gaussian_process_liouville_equation_amd/csrc/gple_g6.h"

static std::vector<uint64_t> table(gple_g6::TABLE_WORDS);

struct Tally
{
	unsigned long long compared = 0, mismatches = 0;
	void one(double v)
	{
		char want[64], got[32];
		const int nw = std::snprintf(want, sizeof want, "%g", v);
		const int ng = gple_g6::format(v, got, table.data());
		++compared;
		if ((ng != nw || std::memcmp(want, got, nw) != 0) && mismatches++ < 5) std::printf("MISMATCH %a: libc '%s', header '%.*s'\n", v, want, ng, got);
	}
	// v and its negative
	void both(double v)
	{
		if (!std::isfinite(v)) return;
		one(v);
		one(-v);
	}
	// v with both neighbours
	void three(double v)
	{
		both(v);
		both(std::nextafter(v, INFINITY));
		both(std::nextafter(v, -INFINITY));
	}
};

// the n-th output of splitmix64 seeded with s0 (its state advances by a constant)
static uint64_t splitmix64(uint64_t s0, uint64_t n)
{
	uint64_t z = s0 + (n + 1) * 0x9e3779b97f4a7c15ull;
	z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
	z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
	return z ^ (z >> 31);
}

int main(int argc, char** argv)
{
	const long random_count = argc > 1 ? std::atol(argv[1]) : 20000000;
	const long tie_stride = std::max(1l, argc > 2 ? std::atol(argv[2]) : 1);
	const int threads = std::max(1, argc > 3 ? std::atoi(argv[3]) : std::min(16, static_cast<int>(std::thread::hardware_concurrency())));
	gple_g6::build_table(table.data());
	// the six-digit prefixes of the tie strings: every tie_stride-th and both ends
	std::vector<long> prefixes;
	for (long D = 100000; D < 999999; D += tie_stride) prefixes.push_back(D);
	prefixes.push_back(999999);
	std::vector<Tally> tally(threads);
	std::vector<std::thread> pool;
	for (int w = 0; w < threads; ++w)
		pool.emplace_back([&, w] {
			Tally& t = tally[w];
			char text[64];
			// random bit patterns
			for (long i = random_count * w / threads; i < random_count * (w + 1) / threads; ++i)
			{
				const uint64_t b = splitmix64(20240607, i);
				double v;
				std::memcpy(&v, &b, sizeof v);
				t.both(v);
			}
			// seven-digit strings D5e<k>: every representable tie, and the doubles next to the ties that are not representable
			const long np = static_cast<long>(prefixes.size());
			for (long i = np * w / threads; i < np * (w + 1) / threads; ++i)
				for (int k = -8; k <= 8; ++k)
				{
					std::snprintf(text, sizeof text, "%ld5e%d", prefixes[i], k);
					t.three(std::strtod(text, nullptr));
				}
			if (w) return;
			t.both(0.0);
			// powers of two
			for (int e = -1074; e <= 1023; ++e) t.three(std::ldexp(1.0, e));
			// decade boundaries, the carry into the next decade, the switches between fixed and exponent style
			for (int k = -330; k <= 310; ++k)
			{
				std::snprintf(text, sizeof text, "1e%d", k);
				t.three(std::strtod(text, nullptr));
				std::snprintf(text, sizeof text, "9.999995e%d", k);
				t.three(std::strtod(text, nullptr));
			}
		});
	for (std::thread& th : pool) th.join();
	Tally sum;
	for (const Tally& t : tally) sum.compared += t.compared, sum.mismatches += t.mismatches;
	std::printf("compared %llu values, %llu mismatches\n", sum.compared, sum.mismatches);
	return sum.mismatches ? 1 : 0;
}
