// trace_jitter.inc -- the reflected ray's jitter (trace.h:77-84): five draws of the pixel's generator, two discarded.
// Textually included by both trace kernels behind trace_bounce.inc.
// Names it uses from the including scope:
//   COUNT, HAS_W, cnt;  ray (the reflected direction).
// Names it writes:
//   iray (the next segment's un-normalised direction; may be an alias of ray), seed.
//@R p_jitter
RG(RG_JITTER);
// trace.h:77-84: five draws, two discarded
// (straight into the next segment's direction)
iray.x = ray.x + lcg2_fs(seed) * REFLECT_BLUR_F;
iray.y = ray.y + lcg2_fs(seed) * REFLECT_BLUR_F;
lcg2_next(seed);
iray.z = ray.z + lcg2_fs(seed) * REFLECT_BLUR_F;
lcg2_next(seed);
if constexpr(HAS_W) iray.w = ray.w;
