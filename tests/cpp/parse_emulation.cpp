// parse_emulation.cpp — csrc/gple_parse.hip compiled for the host (tests/test_parse_host.py), as format_emulation.cpp does for the formatter: every
// thread of a workgroup is a host thread, __syncthreads a barrier, __shfl_up an exchange through memory, atomicMin a locked minimum, workgroups
// run one after another.  It checks what needs no GPU — the pieces' loads at every alignment of the text pointer (the text sits at the very end
// and start of its allocation, so that a sanitized build sees any byte read outside it), token starts and lines across chunk boundaries, both
// scans, the compaction, and that nothing outside values[0 .. count) is written — against strtod on the text split at blanks.
#define __HIP_PLATFORM_AMD__
#include <hip/hip_runtime.h>
#include <algorithm>
#include <barrier>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>
using std::max;
using std::min;
struct Idx { unsigned x = 0, y = 0, z = 0; };
static thread_local Idx threadIdx, blockIdx;
static std::barrier<>* g_bar = nullptr;
static unsigned g_slots[1024];
static std::mutex g_atomic;
inline void __syncthreads() { g_bar->arrive_and_wait(); }
inline unsigned __shfl_up(unsigned v, int d)
{
	const unsigned t = threadIdx.x;
	g_slots[t] = v;
	g_bar->arrive_and_wait();
	const unsigned r = static_cast<int>(t & 63) >= d ? g_slots[t - d] : v;
	g_bar->arrive_and_wait();
	return r;
}
inline unsigned long long atomicMin(unsigned long long* p, unsigned long long v)
{
	std::lock_guard<std::mutex> lk(g_atomic);
	const unsigned long long old = *p;
	*p = std::min(old, v);
	return old;
}
static void emu_launch(unsigned grid, unsigned block, const std::function<void()>& body)
{
	std::barrier<> bar(block);
	g_bar = &bar;
	std::vector<std::thread> ts;
	for (unsigned t = 0; t < block; ++t)
		ts.emplace_back([&, t] {
			for (unsigned b = 0; b < grid; ++b)
			{
				threadIdx.x = t;
				blockIdx.x = b;
				body();
				bar.arrive_and_wait(); // the next workgroup reuses the static "LDS"
			}
		});
	for (auto& th : ts) th.join();
}
#undef __shared__
#define __shared__ static
#undef __launch_bounds__
#define __launch_bounds__(x)
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, grid, block, shm, stream, ...) emu_launch((grid).x, (block).x, [&] { k(__VA_ARGS__); })
#include "../../gaussian_process_liouville_equation_amd/csrc/gple_parse.hip"

static std::vector<uint64_t> table(gple_g6::TABLE_WORDS);
static int bad = 0, cases = 0;
constexpr uint64_t GUARD = 0xABABABABABABABABull;

static bool blank(unsigned char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }

// text at `skew` bytes past a 16-byte boundary, the allocation ending with it; capacity < 0: as many values as the text holds; -2: count only
static void check(const char* name, const std::string& text, int skew, long capacity = -1, long want_bad = -1)
{
	std::vector<uint64_t> want;
	size_t lines = 0;
	bool open = false;
	for (size_t i = 0; i < text.size();)
	{
		if (text[i] == '\n') lines += open, open = false;
		if (blank(text[i]))
		{
			++i;
			continue;
		}
		size_t j = i;
		while (j < text.size() && !blank(text[j])) ++j;
		const double v = std::strtod(text.substr(i, j - i).c_str(), nullptr);
		uint64_t b;
		std::memcpy(&b, &v, 8);
		want.push_back(v != v ? gple_d2::NAN_BITS : b);
		open = true;
		i = j;
	}
	lines += open;
	void* mem = nullptr;
	if (posix_memalign(&mem, 16, skew + text.size() + 1)) std::abort(); // one byte more than the text: never to be read
	unsigned char* at = static_cast<unsigned char*>(mem) + skew;
	std::memcpy(at, text.data(), text.size());
	const bool count_only = capacity == -2;
	const size_t cap = capacity < 0 ? want.size() : static_cast<size_t>(capacity);
	std::vector<uint64_t> values(cap + 2, GUARD);
	std::vector<unsigned char> work(gple::parse_work_bytes(at, text.size()) + 16);
	void* w = work.data() + (16 - reinterpret_cast<uintptr_t>(work.data()) % 16) % 16;
	const unsigned long long* res = nullptr;
	(void)gple::launch_parse(nullptr, reinterpret_cast<const char*>(at), text.size(), reinterpret_cast<const unsigned long long*>(table.data()), w,
		count_only ? nullptr : reinterpret_cast<double*>(values.data() + 1), cap, &res);
	bool ok = res[0] == want.size() && res[1] == lines && values[0] == GUARD && values[cap + 1] == GUARD;
	const bool written = !count_only && want.size() <= cap;
	if (!count_only) ok = ok && res[2] == (want_bad < 0 || !written ? ~0ull : static_cast<unsigned long long>(want_bad));
	for (size_t i = 0; i < cap; ++i)
		if (!written) ok = ok && values[1 + i] == GUARD;
		else if (i < want.size() && want_bad < 0) ok = ok && values[1 + i] == want[i];
	std::free(mem);
	++cases;
	if (!ok) ++bad, std::printf("BAD %s skew %d length %zu: count %llu (want %zu), lines %llu (want %zu), bad offset %lld\n", name, skew, text.size(), res[0], want.size(), res[1], lines, (long long)res[2]);
}

// `length` bytes of numbers that stay numbers wherever a blank cuts them ("123.456000" -> "123.", ".456"), between runs of every kind of blank
static std::string filler(std::mt19937_64& rng, size_t length)
{
	static const char* gaps[] = {" ", " ", " ", "\n", " \n", "\n\n", "\r\n", "\t", "  ", " \v\f ", "\n \t \n"};
	std::string s;
	char buf[64];
	while (s.size() < length)
	{
		std::snprintf(buf, sizeof buf, "%.6f", static_cast<double>(rng() % 100000000) * 1e-5);
		s += buf;
		s += gaps[rng() % (sizeof gaps / sizeof *gaps)];
	}
	s.resize(length);
	return s;
}

int main()
{
	gple_g6::build_table(table.data());
	std::mt19937_64 rng(7);
	const long C = gple::PARSE_CHUNK;
	// lengths around one, two and three chunks; at every alignment of the pointer the chunk boundaries fall at byte k C - skew of the text
	for (long length : {C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1, 3 * C - 1, 3 * C, 3 * C + 1})
		check("length", filler(rng, length), static_cast<int>(length % 5));
	for (int skew = 0; skew < 16; ++skew)
	{
		std::string s = filler(rng, 3 * C + 100);
		for (long k = 1; k <= 3; ++k)
		{
			const long B = k * C - skew; // the first byte of chunk k
			const int kind = (k + skew) % 3;
			if (kind == 0) s.replace(B - 6, 12, " -1.2345e+03"), s[B + 6] = ' '; // a token across the boundary
			else if (kind == 1) s.replace(B - 3, 6, "\n1 2.5"), s[B - 4] = ' ', s[B + 3] = ' ';  // a blank ends the chunk, a token starts the next one
			else s.replace(B - 3, 6, " 77 \n8"), s[B + 3] = ' ';                // a token ends the chunk, a blank starts the next one
		}
		check("boundaries", s, skew);
		if (skew % 7) continue;
		check("boundaries, count only", s, skew, -2);
		// straddling tokens at all three boundaries
		for (long k = 1; k <= 3; ++k) s.replace(k * C - skew - 6, 13, " 6.02214e+23 ");
		check("straddling", s, skew);
	}
	check("empty line runs", "1 2\n\n\n3\n \t \n4 5 6\r\n\r\n7", 3);
	check("leading and trailing blanks", "  \n\n 1.5 -2e3\t\n  ", 5);
	check("no final newline", "1 2 3\n4 5 6", 9);
	check("one token", "42", 15);
	check("empty", "", 0);
	check("empty", "", 11);
	check("all blank", " \n\t \n  ", 2);
	check("all blank, a chunk and more", std::string(C + 7, '\n'), 1);
	check("one line of many blanks", "1" + std::string(2 * C, ' ') + "2\n", 4);
	check("specials", "inf -inf nan -nan +Infinity 1e999 -0 5e-324 2.4703282292062327e-324", 6);
	{
		// capacity one short: nothing written; malformed tokens: the smaller offset, wherever the tokens lie
		const std::string s = filler(rng, 2 * C + 50);
		long tokens = 0;
		for (size_t i = 0; i < s.size(); ++i) tokens += !blank(s[i]) && (i == 0 || blank(s[i - 1]));
		check("capacity one short", s, 7, tokens - 1);
		for (long where : {10l, C - 2, 2 * C + 20})
		{
			std::string t = s;
			t.replace(where, 5, " 1x3 "), t.replace(2 * C + 30, 5, " 0x1 ");
			check("malformed", t, 0, -1, where + 1);
		}
		std::string t = s;
		t.replace(C - 40, 67, " " + std::string(65, '1') + " ");
		check("65 bytes", t, 0, -1, C - 39);
		t = s;
		t.replace(C - 40, 66, " " + std::string(64, '0') + " ");
		check("64 bytes", t, 0);
	}
	std::printf("emulation done, %d cases, %d bad\n", cases, bad);
	return bad != 0;
}
