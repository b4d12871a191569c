// Driver of tests/test_switches_cpu.py: runs its arguments in order against roman_amd/csrc/switches.h.
//   NAME=VALUE  setenv      -NAME  unsetenv      print  read_switches() as one line of  ROMAN_NAME:field=value  words
#include <cstdio>
#include <cstring>
#include <string>

#include "switches.h"

static void print(const roman::Switches& s)
{
    printf("ROMAN_DEBUG:debug=%d ROMAN_WIDE:wide=%d ROMAN_SMALL_FUSED:small_fused=%d ROMAN_SMALL_ONLY:small_only=%d ROMAN_SMALL:small=%d ",
           s.debug, s.wide, s.small_fused, s.small_only, s.small);
    printf("ROMAN_COS_SEL:cos_sel=%d ROMAN_COS_SEL:cos_sel_matrix=%d ROMAN_COS_DEAL:cos_deal=%d ROMAN_COS_BLOCK:cos_block=%d ROMAN_COS_BLOCK:cos_block_large=%d ",
           s.cos_sel, s.cos_sel_matrix, s.cos_deal, s.cos_block, s.cos_block_large);
    printf("ROMAN_COUNT_PRE:count_pre=%d ROMAN_COUNT_WHOLE:count_whole=%d ROMAN_LISTS:lists=%d ROMAN_WIDE_UPPER:wide_upper=%d ROMAN_WIDE_IDX16:wide_idx16=%d ROMAN_COUNT_ZLDS:count_zlds=%d ",
           s.count_pre, s.count_whole, s.lists, s.wide_upper, s.wide_idx16, s.count_zlds);
    printf("ROMAN_SORT_EQMAX:sort_eq_max=%d ROMAN_LISTS_LDS:lists_lds=%d ROMAN_WIDE_TEAMS:wide_teams_set=%d ROMAN_WIDE_TEAMS:wide_teams=%d ROMAN_WIDE_COMPACT:wide_compact_set=%d ROMAN_WIDE_COMPACT:wide_compact=%d ",
           s.sort_eq_max, s.lists_lds, s.wide_teams_set, s.wide_teams, s.wide_compact_set, s.wide_compact);
    printf("ROMAN_TEST_CAPNNZ:test_capnnz_set=%d ROMAN_TEST_CAPNNZ:test_capnnz=%lld ROMAN_TEST_CAPLIST:test_caplist_set=%d ROMAN_TEST_CAPLIST:test_caplist=%lld ",
           s.test_capnnz_set, s.test_capnnz, s.test_caplist_set, s.test_caplist);
    printf("ROMAN_NUM_XCC:num_xcc=%d ROMAN_WIDE_SPIN_MS:wide_spin_ms=%g\n", s.num_xcc, s.wide_spin_ms);
}

int main(int argc, char** argv)
{
    for (int k = 1; k < argc; ++k) {
        const char* a = argv[k];
        const char* eq = strchr(a, '=');
        if (!strcmp(a, "print")) print(roman::read_switches());
        else if (a[0] == '-') unsetenv(a + 1);
        else if (eq) setenv(std::string(a, eq).c_str(), eq + 1, 1);
        else { fprintf(stderr, "bad argument %s\n", a); return 2; }
    }
    return 0;
}
