/* level_host.h -- host-side level helpers of libpwnhip (see level_host.c) */
#ifndef PWN_LEVEL_HOST_H
#define PWN_LEVEL_HOST_H
#include <stdint.h>
#include "pwnhip.h"
#include "cell_bake.h"
#include "sphere_bound.h"
#ifdef __cplusplus
extern "C" {
#endif
void pwn_level_clear(uint8_t *cells, pwn_portal *pmap, int32_t *spawn);
int pwn_parse_level(const char *text, int len, uint8_t *cells, pwn_portal *pmap, int32_t *spawn);
int pwn_check_portals(const uint8_t *cells, const pwn_portal *pmap);
int pwn_bake_cells(const uint8_t *cells, const pwn_portal *pmap, uint16_t *bits, uint32_t *recs);
int pwn_bin_spheres(const pwn_sphere *s, int n, int32_t *off, int32_t *idx, int idx_cap);
int pwn_sphere_bounds_build(const pwn_sphere *s, const int32_t *off, const int32_t *idx, int form, pwn_sphere_bound *out);
#ifdef __cplusplus
}
#endif
#endif
