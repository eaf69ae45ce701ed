// gple_capi_format.hip — C-ABI entry points of include/gple.h: the "%g" text of phase.txt / var.txt, converted on the device (gple_format.hip), and
// read back into doubles there (gple_parse.hip).
#include "gple_capi.h"
#include "gple_d2.h"
#include "gple_debug.h"
#include "gple_g6.h"

namespace
{
	// pooled bytes with scope lifetime (the byte-typed sibling of Staged's buffers)
	struct ByteScratch
	{
		Scratch buf;
		explicit ByteScratch(gple_ctx* c): buf(c) {}
		hipError_t get(size_t bytes) { return buf.get((bytes + sizeof(double) - 1) / sizeof(double)); }
		char* p() const { return reinterpret_cast<char*>(buf.p); }
	};

	// the powers of five: built once per process by repeated multiplication, uploaded once per context
	hipError_t format_table(gple_ctx* ctx)
	{
		if (ctx->format_table) return hipSuccess;
		static const std::vector<uint64_t> host = [] {
			std::vector<uint64_t> t(gple_g6::TABLE_WORDS);
			gple_g6::build_table(t.data());
			return t;
		}();
		void* p = nullptr;
		hipError_t e = hipMalloc(&p, host.size() * sizeof(uint64_t));
		if (e != hipSuccess) return e;
		e = hipMemcpy(p, host.data(), host.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
		if (e != hipSuccess)
		{
			(void)hipFree(p);
			return e;
		}
		ctx->format_table = static_cast<unsigned long long*>(p);
		return hipSuccess;
	}
} // namespace

extern "C"
{
	/* the most the text of gple_format_g can take: a blank and 13 bytes per number ("-1.23457e-308") and the newlines */
	size_t gple_format_g_bound(size_t count, size_t per_line, size_t lines_per_block)
	{
		const size_t lines = per_line ? count / per_line : 0;
		return (gple_g6::MAX_BYTES + 1) * count + lines + (lines_per_block ? lines / lines_per_block : 0);
	}

	/* replaces the stream output of output_phase_space_distribution (general.cpp:384-392) and of output_phase (output.cpp:180-232) */
	int gple_format_g(gple_ctx* ctx, const double* values, size_t count, size_t per_line, size_t lines_per_block, unsigned flags, char* text,
		size_t capacity, size_t* length)
	{
		if (!ctx || !length || per_line == 0 || count % per_line != 0 || count > FORMAT_MAX_COUNT ||
			capacity < gple_format_g_bound(count, per_line, lines_per_block) || (count && (!values || !text)))
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (count == 0)
		{
			*length = 0;
			return GPLE_OK;
		}
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		hipStream_t st = ctx->stream;
		GPLE_HIP(ctx, format_table(ctx));
		Staged v(ctx, dev);
		ByteScratch work(ctx), staged_text(ctx);
		GPLE_HIP(ctx, v.in(values, count));
		GPLE_HIP(ctx, work.get(format_work_bytes(count, ctx->format_slots)));
		char* out = text;
		if (!dev)
		{
			GPLE_HIP(ctx, staged_text.get(gple_format_g_bound(count, per_line, lines_per_block)));
			out = staged_text.p();
		}
		const unsigned long long* length_dev = nullptr;
		timer_start(ctx, GPLE_TIMER_FORMAT);
		GPLE_HIP(ctx, launch_format(st, v.p, count, per_line, lines_per_block, (flags & GPLE_FORMAT_JOIN) != 0, ctx->format_table, work.p(),
			ctx->format_slots, out, &length_dev));
		timer_stop(ctx, GPLE_TIMER_FORMAT);
		unsigned long long bytes = 0;
		GPLE_HIP(ctx, hipMemcpyAsync(&bytes, length_dev, sizeof(bytes), hipMemcpyDeviceToHost, st));
		GPLE_HIP(ctx, hipStreamSynchronize(st));
		if (!dev) GPLE_HIP(ctx, hipMemcpy(text, out, bytes, hipMemcpyDeviceToHost));
		*length = bytes;
		return GPLE_OK;
	}

	/* replaces the stream extraction of read_density (test/io.cpp:25-72) */
	int gple_parse_g(gple_ctx* ctx, const char* text, size_t length, unsigned flags, double* values, size_t capacity, size_t* count, size_t* lines,
		size_t* bad_offset)
	{
		if (!ctx || !count || (length && !text) || length > PARSE_MAX_LENGTH || (!values && capacity)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (bad_offset) *bad_offset = static_cast<size_t>(-1);
		if (length == 0)
		{
			*count = 0;
			if (lines) *lines = 0;
			return GPLE_OK;
		}
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		hipStream_t st = ctx->stream;
		GPLE_HIP(ctx, format_table(ctx));
		ByteScratch work(ctx), staged_text(ctx);
		Staged v(ctx, dev);
		const char* in = text;
		if (!dev)
		{
			GPLE_HIP(ctx, staged_text.get(length));
			GPLE_HIP(ctx, hipMemcpyAsync(staged_text.p(), text, length, hipMemcpyHostToDevice, st));
			in = staged_text.p();
		}
		GPLE_HIP(ctx, v.out(values, capacity));
		GPLE_HIP(ctx, work.get(parse_work_bytes(in, length)));
		const unsigned long long* result_dev = nullptr;
		timer_start(ctx, GPLE_TIMER_PARSE);
		GPLE_HIP(ctx, launch_parse(st, in, length, ctx->format_table, work.p(), v.p, capacity, &result_dev));
		timer_stop(ctx, GPLE_TIMER_PARSE);
		unsigned long long result[3] = {0, 0, 0};
		GPLE_HIP(ctx, hipMemcpyAsync(result, result_dev, sizeof(result), hipMemcpyDeviceToHost, st));
		GPLE_HIP(ctx, hipStreamSynchronize(st));
		*count = result[0];
		if (lines) *lines = result[1];
		if (!values) return GPLE_OK;
		if (result[0] > capacity)
		{
			ctx->last_error = "gple_parse_g: the text holds " + std::to_string(result[0]) + " numbers, capacity is " + std::to_string(capacity);
			return GPLE_ERR_BAD_ARG;
		}
		if (result[2] != ~0ull)
		{
			char token[gple_d2::MAX_TOKEN + 1];
			const size_t n = std::min<size_t>(sizeof(token), length - result[2]);
			GPLE_HIP(ctx, hipMemcpy(token, in + result[2], n, hipMemcpyDeviceToHost));
			size_t end = 0;
			while (end < n && !gple_d2::is_blank(static_cast<unsigned char>(token[end]))) ++end;
			if (bad_offset) *bad_offset = result[2];
			ctx->last_error = "gple_parse_g: malformed token '" + std::string(token, end) + (end == sizeof(token) ? "...'" : "'") + " at byte " + std::to_string(result[2]);
			return GPLE_ERR_BAD_ARG;
		}
		if (!dev) GPLE_HIP(ctx, hipMemcpy(values, v.p, result[0] * sizeof(double), hipMemcpyDeviceToHost));
		return GPLE_OK;
	}

	int gple_debug_format_knobs(gple_ctx* ctx, int slots)
	{
		if (!ctx) return GPLE_ERR_BAD_ARG;
		std::lock_guard<std::mutex> lk(ctx->call_mu);
		if (slots >= 0) ctx->format_slots = slots != 0;
		return GPLE_OK;
	}
}
