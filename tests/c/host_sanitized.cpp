/*
 * host_sanitized.cpp -- the library's host statements, size rules, constructors, designs and planners under AddressSanitizer and
 * UndefinedBehaviorSanitizer (tests/test_host_sanitized_cpu.py builds the library's sources with the sanitizers and links them here)
 *
 *   host_sanitized <cases> <results>
 *
 * Every entry point called here takes no struct fosphor * and needs no device; no HIP function is called.  <cases> is a list of
 * calls (little endian):
 *   u32 n_cases, then per case   u16 name length, the name, u32 n_args, then per argument one byte of kind and
 *       0  an integer     i64
 *       1  a real         f64
 *       2  a NULL pointer
 *       3  a buffer       u64 size, then its bytes
 * The rule for buffers: every buffer lies in a heap allocation of its own of exactly `size` bytes -- what the header's contract
 * promises the callee and not a byte more -- so that the sanitizer's red zones stand where a read or write one element past the
 * contract lands.  Nothing is shared between the arguments of a call or between calls.
 * <results> gets per case the return value (8 bytes: an integer as i64, a double as its bits, a float as its bits zero-extended,
 * a string as its length; void as 0) and then every buffer of the call as the callee left it, in argument order.  The case's index
 * and name go to stderr before the call, so that a sanitizer report names its case.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "fosphor.h"
#include "fosphor_amd.h"
#include "fosphor_amd_axis.h"
#include "fosphor_amd_burst.h"
#include "fosphor_amd_carrier.h"
#include "fosphor_amd_cmap.h"
#include "fosphor_amd_correlate.h"
#include "fosphor_amd_decide.h"
#include "fosphor_amd_decode.h"
#include "fosphor_amd_demod.h"
#include "fosphor_amd_detect.h"
#include "fosphor_amd_extract.h"
#include "fosphor_amd_mask.h"
#include "fosphor_amd_measure.h"
#include "fosphor_amd_psd.h"
#include "fosphor_amd_resample.h"
#include "fosphor_amd_soft.h"
#include "fosphor_amd_symbols.h"
#include "fosphor_amd_view.h"

namespace {

struct Arg {
	int kind;
	int64_t i;
	double d;
	size_t size;
	void *p;		/* malloc(size): the buffer and nothing else */
};

struct Reader {
	FILE *f;
	template <class T> T get()
	{
		T v;
		if (fread(&v, sizeof v, 1, f) != 1) {
			fprintf(stderr, "host_sanitized: the case file ends early\n");
			exit(2);
		}
		return v;
	}
};

template <class T>
T as(const Arg &a)
{
	if constexpr (std::is_pointer<T>::value) {
		if (a.kind != 2 && a.kind != 3) {
			fprintf(stderr, "host_sanitized: a pointer argument needs a buffer or NULL\n");
			exit(2);
		}
		return reinterpret_cast<T>(a.kind == 3 ? a.p : nullptr);
	} else if constexpr (std::is_floating_point<T>::value) {
		return static_cast<T>(a.kind == 1 ? a.d : (double)a.i);
	} else {
		static_assert(std::is_integral<T>::value, "an argument that is neither pointer, real nor integer");
		if (a.kind != 0) {
			fprintf(stderr, "host_sanitized: an integer argument needs an integer\n");
			exit(2);
		}
		return static_cast<T>(a.i);
	}
}

template <class R>
uint64_t bits_of(R r)
{
	uint64_t b = 0;
	if constexpr (std::is_same<R, const char *>::value)
		b = r ? strlen(r) : 0;
	else if constexpr (std::is_integral<R>::value)
		b = (uint64_t)(int64_t)r;
	else
		memcpy(&b, &r, sizeof r);
	return b;
}

template <class R, class... A, size_t... I>
uint64_t invoke(R (*fn)(A...), const std::vector<Arg> &args, std::index_sequence<I...>)
{
	if (args.size() != sizeof...(A)) {
		fprintf(stderr, "host_sanitized: %zu arguments where the entry point takes %zu\n", args.size(), sizeof...(A));
		exit(2);
	}
	if constexpr (std::is_void<R>::value) {
		fn(as<A>(args[I])...);
		return 0;
	} else {
		return bits_of<R>(fn(as<A>(args[I])...));
	}
}

template <class R, class... A>
uint64_t call(R (*fn)(A...), const std::vector<Arg> &args)
{
	return invoke(fn, args, std::index_sequence_for<A...>());
}

typedef uint64_t (*Entry)(const std::vector<Arg> &);

#define ENTRY(name) { #name, [](const std::vector<Arg> &a) { return call(&name, a); } }

const std::map<std::string, Entry> kEntries = {
	/* the host statements */
	ENTRY(fosphor_amd_extract_host), ENTRY(fosphor_amd_measure_host), ENTRY(fosphor_amd_demod_host),
	ENTRY(fosphor_amd_correlate_host), ENTRY(fosphor_amd_resample_host), ENTRY(fosphor_amd_psd_host),
	ENTRY(fosphor_amd_symbols_host), ENTRY(fosphor_amd_carrier_host), ENTRY(fosphor_amd_decide_host),
	ENTRY(fosphor_amd_decode_host), ENTRY(fosphor_amd_soft_host),
	ENTRY(fosphor_amd_bursts_host), ENTRY(fosphor_amd_mask_row_host), ENTRY(fosphor_amd_detect_bands_host),
	/* the size rules */
	ENTRY(fosphor_amd_demod_n_out), ENTRY(fosphor_amd_correlate_n_out), ENTRY(fosphor_amd_resample_n_out),
	ENTRY(fosphor_amd_psd_n_seg), ENTRY(fosphor_amd_symbols_max_out), ENTRY(fosphor_amd_decode_steps),
	/* the constructors */
	ENTRY(fosphor_amd_extract_from_burst), ENTRY(fosphor_amd_measure_from_extract), ENTRY(fosphor_amd_demod_from_extract),
	ENTRY(fosphor_amd_correlate_from_extract), ENTRY(fosphor_amd_resample_from_extract), ENTRY(fosphor_amd_psd_from_extract),
	ENTRY(fosphor_amd_symbols_from_extract), ENTRY(fosphor_amd_symbols_from_resample), ENTRY(fosphor_amd_carrier_from_symbols),
	ENTRY(fosphor_amd_decide_from_carrier), ENTRY(fosphor_amd_decode_from_decide), ENTRY(fosphor_amd_soft_from_decide),
	ENTRY(fosphor_amd_view_from_render),
	/* the designs */
	ENTRY(fosphor_amd_extract_design), ENTRY(fosphor_amd_resample_design), ENTRY(fosphor_amd_resample_ratio),
	ENTRY(fosphor_amd_psd_window), ENTRY(fosphor_amd_psd_twiddles), ENTRY(fosphor_amd_symbols_twiddles),
	/* the records as values */
	ENTRY(fosphor_amd_measure_derive), ENTRY(fosphor_amd_correlate_derive), ENTRY(fosphor_amd_psd_derive),
	ENTRY(fosphor_amd_symbols_derive), ENTRY(fosphor_amd_carrier_derive), ENTRY(fosphor_amd_decide_derive),
	ENTRY(fosphor_amd_decode_derive), ENTRY(fosphor_amd_soft_derive),
	/* the rest */
	ENTRY(fosphor_amd_view_span), ENTRY(fosphor_amd_mask_from_points), ENTRY(fosphor_amd_detect_bin_y),
	ENTRY(fosphor_amd_cmap_generate), ENTRY(fosphor_amd_freq_axis_build), ENTRY(fosphor_amd_freq_axis_render),
	ENTRY(fosphor_amd_host_thresholds), ENTRY(fosphor_amd_host_twiddle_count), ENTRY(fosphor_amd_host_twiddles),
	ENTRY(fosphor_amd_plan_piece_batches), ENTRY(fosphor_amd_plan_count), ENTRY(fosphor_amd_plan_k1),
	ENTRY(fosphor_amd_demod_atan2_turns), ENTRY(fosphor_amd_demod_atan2_turns_n), ENTRY(fosphor_amd_carrier_cossin_turns),
	ENTRY(fosphor_amd_carrier_cossin_turns_n), ENTRY(fosphor_amd_psd_ratio_from_db), ENTRY(fosphor_amd_version),
};

} // namespace

int main(int argc, char **argv)
{
	if (argc != 3) {
		fprintf(stderr, "usage: host_sanitized <cases> <results>\n");
		return 2;
	}
	FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
	if (!in || !out) {
		fprintf(stderr, "host_sanitized: cannot open %s or %s\n", argv[1], argv[2]);
		return 2;
	}
	Reader r = { in };
	const uint32_t n_cases = r.get<uint32_t>();
	for (uint32_t c = 0; c < n_cases; c++) {
		std::string name(r.get<uint16_t>(), '\0');
		if (!name.empty() && fread(&name[0], name.size(), 1, in) != 1)
			return 2;
		std::vector<Arg> args(r.get<uint32_t>());
		for (Arg &a : args) {
			a = Arg();
			a.kind = r.get<uint8_t>();
			if (a.kind == 0)
				a.i = r.get<int64_t>();
			else if (a.kind == 1)
				a.d = r.get<double>();
			else if (a.kind == 3) {
				a.size = (size_t)r.get<uint64_t>();
				a.p = malloc(a.size);
				if (!a.p || (a.size && fread(a.p, a.size, 1, in) != 1)) {
					fprintf(stderr, "host_sanitized: case %u: no buffer of %zu bytes\n", c, a.size);
					return 2;
				}
			} else if (a.kind != 2) {
				fprintf(stderr, "host_sanitized: case %u: argument kind %d\n", c, a.kind);
				return 2;
			}
		}
		const auto e = kEntries.find(name);
		if (e == kEntries.end()) {
			fprintf(stderr, "host_sanitized: case %u: no entry point %s\n", c, name.c_str());
			return 2;
		}
		fprintf(stderr, "case %u %s\n", c, name.c_str());
		const uint64_t rv = e->second(args);
		fwrite(&rv, sizeof rv, 1, out);
		for (Arg &a : args)
			if (a.kind == 3) {
				if (a.size)
					fwrite(a.p, a.size, 1, out);
				free(a.p);
			}
	}
	if (fclose(out))
		return 2;
	fclose(in);
	fprintf(stderr, "done %u\n", n_cases);
	return 0;
}
