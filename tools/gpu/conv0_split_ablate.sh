# timing-only ablation build of the persistent split conv0 (wrong results by design): 71 no MFMA phase (producers alone)
cd $GRAFT_REPO_ROOT
C=$GRAFT_REPO_ROOT/scene_3dreconstruction_mvsnet_amd/csrc
for r in 1 2; do
python tools/time_stage.py conv0 300
MVS_LIB_PATH=$C/libmvs_hip_ablate71.so python tools/time_stage.py conv0 300
done
