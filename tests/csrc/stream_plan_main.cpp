// Prints the stream plan of a mapping context (airlift_amd/csrc/al_stream_plan.h) for every number of physical streams, and the
// rule that picks that number: a stand-alone program of host code only (tests/test_stream_plan_cpu.py builds it with
// AddressSanitizer + UBSan and reads what it prints).
#include <stdio.h>
#include "al_stream_plan.h"

int main()
{
	printf("roles %d\n", (int)AL_ROLE_N);
	for (int n = 1; n <= AL_ROLE_N; ++n) {
		uint8_t map[AL_ROLE_N];
		al_stream_plan(n, map);            // (asserts the header's own conditions)
		printf("plan %d", n);
		for (int r = 0; r < AL_ROLE_N; ++r) printf(" %d", (int)map[r]);
		printf("\n");
	}
	for (int k = 0; k < AL_N_NEVER_TOGETHER; ++k) printf("apart %d %d\n", (int)AL_NEVER_TOGETHER[k].a, (int)AL_NEVER_TOGETHER[k].b);
	static const char *const cases[][2] = {{nullptr, nullptr}, {nullptr, "4"}, {nullptr, "16"}, {nullptr, "2"}, {nullptr, "0"}, {nullptr, "x"}, {"1", "16"}, {"6", nullptr}, {"10", "4"}, {"99", nullptr}, {"0", "8"}, {"-3", nullptr}};
	for (const auto &cs : cases) {
		int src = -1; const int n = al_stream_count(cs[0], cs[1], &src);
		printf("count %s %s -> %d %d\n", cs[0] ? cs[0] : "-", cs[1] ? cs[1] : "-", n, src);
	}
	static const char *const maps[] = {"0,1,2,3,1,1,2,2,3,3", "0,0,0,0,0,0,0,0,0,0", "0,1,2,3,4,5,6,7,8,9", "0,1,2,3,1,1,2,2,3", "0,1,2,3,1,1,2,2,3,3,1", "0,1,2,4,1,1,2,2,4,4", "1,0,2,3,1,1,2,2,3,3",
	                                   "0,0,2,1,1,1,2,2,1,1", "0,1,2,3,1,1,2,2,3,x", "0,1,2,3,1,1,2,2,3,12", "", nullptr};
	for (const char *m : maps) { uint8_t map[AL_ROLE_N] = {}; printf("parse %s -> %d\n", m ? (*m ? m : "empty") : "-", al_stream_map_parse(m, map)); }
	return 0;
}
