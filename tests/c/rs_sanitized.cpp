/*
 * rs_sanitized.cpp -- the host side of the Reed-Solomon pass (include/fosphor_amd_rs.h) under AddressSanitizer and
 * UndefinedBehaviorSanitizer: tests/test_rs_sanitized_cpu.py compiles this file and gr-fosphor_amd/csrc/fosphor_rs_host.cpp, and
 * nothing else, with the sanitizers and runs
 *
 *   rs_sanitized <cases> <results>
 *
 * No device, no instance, no HIP function.  <cases> is a list of calls (little endian): u32 n_calls, then per call a byte of kind
 *   0  fosphor_amd_rs_host          i64 n_bytes, i32 n_jobs, i64 out_capacity, u8 nulls, buffers in, jobs; sizes records, out
 *   1  fosphor_amd_rs_encode_host   i64 data_capacity, i32 n_jobs, i64 n_bytes, u8 nulls, buffers data, jobs; size frames
 *   2  fosphor_amd_rs_from_decode   i64 out_offset, i32 n_bits, i64 skip_bytes, i32 n_code, i32 depth, u8 nulls
 * A buffer is u64 size and its bytes, a size is u64.  Bit i of nulls makes pointer i of the call NULL.  The rule for buffers:
 * every buffer lies in a heap allocation of its own of exactly `size` bytes -- what the header's contract promises the callee and
 * not a byte more -- so that the sanitizer's red zones stand where a read or write one byte past the contract lands.  Outputs
 * are filled with 0xa5 first.  <results> gets per call the return value (i32) and then every output of the call as the callee
 * left it.  The call's index goes to stderr before the call, so that a sanitizer report names its case.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fosphor_amd_rs.h"

namespace {

FILE *in_file, *out_file;

template <class T> T get()
{
	T v;
	if (fread(&v, sizeof v, 1, in_file) != 1) {
		fprintf(stderr, "rs_sanitized: the case file ends early\n");
		exit(2);
	}
	return v;
}

/* an allocation of exactly `size` bytes (of one byte where size is 0: never read), read from the file or filled with 0xa5 */
struct Buffer {
	uint8_t *p;
	size_t size;
	Buffer(bool from_file)
	{
		size = (size_t)get<uint64_t>();
		p = static_cast<uint8_t *>(malloc(size ? size : 1));
		if (!p)
			exit(2);
		if (from_file) {
			if (size && fread(p, 1, size, in_file) != size)
				exit(2);
		} else {
			memset(p, 0xa5, size);
		}
	}
	~Buffer() { free(p); }
	void put() const
	{
		if (size && fwrite(p, 1, size, out_file) != size)
			exit(2);
	}
	template <class T> T *as(int nulls, int bit) const { return ((nulls >> bit) & 1) ? nullptr : reinterpret_cast<T *>(p); }
};

void put_rv(int rv)
{
	const int32_t v = rv;
	if (fwrite(&v, sizeof v, 1, out_file) != 1)
		exit(2);
}

} // namespace

int main(int argc, char **argv)
{
	if (argc != 3)
		return 2;
	in_file = fopen(argv[1], "rb");
	out_file = fopen(argv[2], "wb");
	if (!in_file || !out_file)
		return 2;
	const uint32_t n_calls = get<uint32_t>();
	for (uint32_t i = 0; i < n_calls; i++) {
		const int kind = get<uint8_t>();
		fprintf(stderr, "case %u kind %d\n", i, kind);
		if (kind == 0) {
			const int64_t n_bytes = get<int64_t>();
			const int32_t n_jobs = get<int32_t>();
			const int64_t cap = get<int64_t>();
			const int nulls = get<uint8_t>();
			Buffer in(true), jobs(true), records(false), out(false);
			put_rv(fosphor_amd_rs_host(in.as<const uint8_t>(nulls, 0), n_bytes, jobs.as<const struct fosphor_amd_rs_job>(nulls, 1), n_jobs,
			                           records.as<struct fosphor_amd_rs_record>(nulls, 2), out.as<uint8_t>(nulls, 3), cap));
			records.put();
			out.put();
		} else if (kind == 1) {
			const int64_t cap = get<int64_t>();
			const int32_t n_jobs = get<int32_t>();
			const int64_t n_bytes = get<int64_t>();
			const int nulls = get<uint8_t>();
			Buffer data(true), jobs(true), frames(false);
			put_rv(fosphor_amd_rs_encode_host(data.as<const uint8_t>(nulls, 0), cap, jobs.as<const struct fosphor_amd_rs_job>(nulls, 1), n_jobs,
			                                  frames.as<uint8_t>(nulls, 2), n_bytes));
			frames.put();
		} else if (kind == 2) {
			const int64_t out_offset = get<int64_t>();
			const int32_t n_bits = get<int32_t>();
			const int64_t skip = get<int64_t>();
			const int32_t n_code = get<int32_t>(), depth = get<int32_t>();
			const int nulls = get<uint8_t>();
			struct fosphor_amd_rs_job *job = static_cast<struct fosphor_amd_rs_job *>(malloc(sizeof *job));
			if (!job)
				return 2;
			memset(job, 0xa5, sizeof *job);
			put_rv(fosphor_amd_rs_from_decode(out_offset, n_bits, skip, n_code, depth, (nulls & 1) ? nullptr : job));
			if (fwrite(job, sizeof *job, 1, out_file) != 1)
				return 2;
			free(job);
		} else {
			fprintf(stderr, "rs_sanitized: kind %d\n", kind);
			return 2;
		}
	}
	fclose(in_file);
	if (fclose(out_file))
		return 2;
	fprintf(stderr, "done %u\n", n_calls);
	return 0;
}
